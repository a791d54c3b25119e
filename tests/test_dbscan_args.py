"""The DBSCAN entries without a GPU: the ABI names, every argument error before any HIP call, the workspace sizes, and the
Python argument checks."""
import ctypes

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import _lib

NEW = ["mi355_dbscan_workspace_bytes", "mi355_dbscan_f16_workspace_bytes", "mi355_dbscan_init", "mi355_dbscan_degree",
       "mi355_dbscan_degree_f16", "mi355_dbscan_link", "mi355_dbscan_link_f16", "mi355_dbscan_finish"]
P = 0x1000        # a non-null, 16-byte aligned address that no check may dereference
BIG = (1 << 31) - 128


def test_new_entries_are_declared_bound_and_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name
    assert _lib.lib().mi355_abi_version() == 3
    assert M.dbscan is M.cluster.dbscan and M.connected_components is M.cluster.connected_components
    assert M.DBSCANResult._fields == ("labels", "core", "degree", "roots", "counts", "n_clusters", "n_noise")
    assert hasattr(M.Gallery, "dbscan") and hasattr(M.Gallery, "components")


def _fails(status, word):
    msg = _lib.lib().mi355_last_error()
    assert status != 0 and word.encode() in msg, (status, msg)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("link", [False, True])
def test_sweep_argument_errors(f16, link):
    L = _lib.lib()

    def call(q=P, q0=0, rows=4, g=P, N=10, dim=8, thr=0.5, ms=2, deg=P, par=P, bor=P, ws=P, wsb=1 << 30):
        norm = () if f16 else (1,)
        state = (ms, deg, par, bor) if link else (deg,)
        name = "mi355_dbscan_" + ("link" if link else "degree") + ("_f16" if f16 else "")
        return getattr(L, name)(q, q0, rows, g, N, dim, *norm, 1e-6, thr, *state, ws, wsb, None)
    _fails(call(q=None), "null")
    _fails(call(g=None), "null")
    _fails(call(deg=None), "null degree")
    _fails(call(N=0), "bad shape")
    _fails(call(dim=0), "bad shape")
    _fails(call(N=BIG, rows=1), "too large")
    _fails(call(q0=-1), "outside")
    _fails(call(rows=-1), "outside")
    _fails(call(q0=8, rows=3), "outside")
    _fails(call(q0=11, rows=0), "outside")
    _fails(call(thr=float("nan")), "not finite")
    _fails(call(thr=float("inf")), "not finite")
    _fails(call(deg=P + 2), "aligned")
    _fails(call(ws=None), "workspace")
    _fails(call(wsb=16), "workspace")
    if link:
        _fails(call(par=None), "null parent/border")
        _fails(call(bor=None), "null parent/border")
        _fails(call(ms=0), "min_samples")
        _fails(call(ms=-3), "min_samples")
        _fails(call(par=P + 1), "aligned")
        _fails(call(bor=P + 4), "aligned")
    if f16:
        _fails(call(g=P + 8), "16-byte aligned")


def test_init_and_finish_argument_errors():
    L = _lib.lib()
    _fails(L.mi355_dbscan_init(0, P, P, P, None), "N=")
    _fails(L.mi355_dbscan_init(BIG, P, P, P, None), "N=")
    for k in range(3):
        args = [P, P, P]
        args[k] = None
        _fails(L.mi355_dbscan_init(10, *args, None), "null")
    _fails(L.mi355_dbscan_init(10, P + 2, P, P, None), "aligned")
    _fails(L.mi355_dbscan_init(10, P, P, P + 4, None), "aligned")

    def finish(N=10, ms=1, deg=P, par=P, bor=P, root=P, core=P):
        return L.mi355_dbscan_finish(N, ms, deg, par, bor, root, core, None)
    _fails(finish(N=0), "N=")
    _fails(finish(N=BIG), "N=")
    _fails(finish(ms=0), "min_samples")
    for kw in ("deg", "par", "bor"):
        _fails(finish(**{kw: None}), "null degree/parent/border")
    for kw in ("root", "core"):
        _fails(finish(**{kw: None}), "null root/core")
    _fails(finish(par=P + 2), "aligned")
    _fails(finish(root=P + 4), "aligned")


def test_workspace_sizes():
    L = _lib.lib()
    for fn in (L.mi355_dbscan_workspace_bytes, L.mi355_dbscan_f16_workspace_bytes):
        assert fn(0, 10, 8) == 0 and fn(4, 0, 8) == 0 and fn(4, 10, 0) == 0
        assert fn(4096, 100000, 1536) > 4096 * 1536 * 4                        # the normalised queries of one block
        assert fn(4096, 100000, 1536) < 64 * 2**20                             # no slab, no pair list, no table per tile
    # the sweep's scratch is that of the other searches without a top-k: the same carve
    assert L.mi355_dbscan_workspace_bytes(300, 5000, 70) == L.mi355_roc_pairs_workspace_bytes(300, 5000, 70)
    assert L.mi355_dbscan_f16_workspace_bytes(300, 5000, 70) == L.mi355_roc_pairs_f16_workspace_bytes(300, 5000, 70)


def test_python_argument_checks_need_no_gpu():
    x = torch.zeros(6, 4)
    for call in (lambda: M.dbscan(x, 0.5), lambda: M.connected_components(x, 0.5)):
        with pytest.raises(M.MI355Error, match="GPU"):
            call()
    with pytest.raises(M.MI355Error):
        M.dbscan("rows", 0.5)


def test_checks_come_before_any_launch(monkeypatch):
    # pretend the tensors are on the GPU: every call below must raise on its arguments before it reaches the library
    from imageretrievalresearch_amd import cluster, rank
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)
    monkeypatch.setattr(cluster, "require_cuda", lambda t, name: None)
    monkeypatch.setattr(cluster, "lib", lambda: pytest.fail("reached the library"))
    monkeypatch.setattr(rank, "lib", lambda: pytest.fail("reached the library"))
    x = torch.zeros(6, 4)
    for t in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(M.MI355Error, match="threshold"):
            M.dbscan(x, t)
        with pytest.raises(M.MI355Error, match="threshold"):
            M.connected_components(x, t)
    for ms in (0, -1, 2.0, True, None):
        with pytest.raises(M.MI355Error, match="min_samples"):
            M.dbscan(x, 0.5, ms)
    for b in (0, -4, 1.5, True):
        with pytest.raises(M.MI355Error, match="block"):
            M.dbscan(x, 0.5, 2, block=b)
    with pytest.raises(M.MI355Error):
        M.dbscan(torch.zeros(6), 0.5)
    with pytest.raises(TypeError):
        M.connected_components(x, 0.5, min_samples=2)                          # components are min_samples = 1
    empty = M.dbscan(torch.zeros(0, 4), 0.5, 3)                                 # no rows: an empty result, no launch
    assert isinstance(empty, M.DBSCANResult) and empty.n_clusters == 0 and empty.n_noise == 0
    assert empty.labels.shape == (0,) and empty.labels.dtype == torch.int64 and empty.core.dtype == torch.bool
    assert empty.degree.shape == empty.roots.shape == empty.counts.shape == (0,)
    g = M.Gallery.__new__(M.Gallery)
    g._buf, g.rows, g.dim, g.eps, g._prepared, g._prepared_rows = torch.zeros(6, 4), 6, 4, 1e-6, None, 0
    with pytest.raises(M.MI355Error, match="min_samples"):
        g.dbscan(0.5, 0)
    with pytest.raises(M.MI355Error, match="threshold"):
        g.components(float("nan"))
