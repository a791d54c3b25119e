"""Diffusion re-ranking without a GPU: the new symbols are declared, bound and exported; every guard of the mi355_diffusion_*
entries (rejected before any HIP call, with a message) and of the Python API; the LDS sizer; and where the public names live."""
import ctypes
import math

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib, diffusion as D
from imageretrievalresearch_amd import rank as R

NAMES = ["mi355_diffusion_graph", "mi355_diffusion_lds_bytes", "mi355_diffusion_solve", "mi355_diffusion_source"]


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_are_declared_bound_and_exported():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert _lib.lib().mi355_abi_version() == 3


def _graph(nn=1, nv=1, G=100, kd=5, gamma=3, cols=1, vals=1, deg=1):
    return _lib.lib().mi355_diffusion_graph(nn, nv, G, kd, gamma, cols, vals, deg, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(nn=None), b"null"), (dict(nv=None), b"null"), (dict(cols=None), b"null"), (dict(vals=None), b"null"), (dict(deg=None), b"null"),
    (dict(kd=0), b"kd=0"), (dict(kd=33), b"kd=33"), (dict(G=5), b"G=5"), (dict(G=0), b"G=0"), (dict(G=1 << 31), b"G="),
    (dict(gamma=0), b"gamma=0"), (dict(gamma=9), b"gamma=9"),
])
def test_graph_entry_rejects_bad_arguments(kw, msg):
    assert _graph(**kw) != 0
    assert msg in _err(), (kw, _err())


def _source(sv=1, si=1, Q=4, L=64, kq=5, gamma=3, y=1):
    return _lib.lib().mi355_diffusion_source(sv, si, Q, L, kq, gamma, y, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(sv=None), b"null"), (dict(si=None), b"null"), (dict(y=None), b"null"), (dict(Q=-1), b"Q=-1"), (dict(L=0), b"L=0"),
    (dict(L=1025), b"L=1025"), (dict(kq=0), b"kq=0"), (dict(kq=65), b"kq=65"), (dict(gamma=0), b"gamma=0"), (dict(gamma=9), b"gamma=9"),
])
def test_source_entry_rejects_bad_arguments(kw, msg):
    assert _source(**kw) != 0
    assert msg in _err(), (kw, _err())


def _solve(cols=1, vals=1, G=100, kd=5, si=1, y=1, Q=4, L=64, alpha=0.99, iters=20, f=1, its=None):
    return _lib.lib().mi355_diffusion_solve(cols, vals, G, kd, si, y, Q, L, alpha, iters, f, its, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(cols=None), b"null"), (dict(vals=None), b"null"), (dict(si=None), b"null"), (dict(y=None), b"null"), (dict(f=None), b"null"),
    (dict(kd=0), b"kd=0"), (dict(kd=33), b"kd=33"), (dict(G=0), b"G=0"), (dict(Q=-1), b"Q=-1"), (dict(L=0), b"L=0"),
    (dict(L=1025), b"L=1025"), (dict(iters=0), b"iters=0"), (dict(iters=65), b"iters=65"), (dict(alpha=0.0), b"alpha"),
    (dict(alpha=1.0), b"alpha"), (dict(alpha=-0.5), b"alpha"), (dict(alpha=math.nan), b"alpha"), (dict(alpha=math.inf), b"alpha"),
])
def test_solve_entry_rejects_bad_arguments(kw, msg):
    assert _solve(**kw) != 0
    assert msg in _err(), (kw, _err())


def test_zero_queries_do_nothing():
    assert _source(Q=0) == 0 and _solve(Q=0) == 0


def test_lds_sizer():
    size = _lib.lib().mi355_diffusion_lds_bytes
    top = size(1024, 32)
    assert 1024 * 32 * 2 < top <= 160 * 1024                     # the uint16 positions alone are 64 KB
    assert D.lds_bytes(1024, 32) == top
    assert 0 < size(1, 1) < size(64, 8) < size(257, 32) < top
    for L, kd in ((0, 5), (1025, 5), (64, 0), (64, 33), (-1, -1)):
        assert size(L, kd) == 0, (L, kd)


def test_python_parameters():
    assert D.diffusion_params(3000, 5) == (5, 20, 10, 0.99, 3, 20, 200)
    assert D.diffusion_params(150, 5) == (5, 20, 10, 0.99, 3, 20, 150)            # shortlist default: min(G, max(k, 200))
    assert D.diffusion_params(3000, 250)[6] == 250
    assert D.diffusion_params(40, 40, kd=32, kq=40, alpha=0.5, gamma=8, iters=64, shortlist=40) == (40, 32, 40, 0.5, 8, 64, 40)
    assert D.diffusion_params(3000, 1, kd=1, kq=1, gamma=1, iters=1, shortlist=1024)[6] == 1024
    assert D.index_params(300) == (20, 3)
    for kw in (dict(kd=0), dict(kd=33), dict(kd=True), dict(kd=2.0), dict(kq=0), dict(kq=201), dict(kq=1.0), dict(gamma=0),
               dict(gamma=9), dict(gamma=3.0), dict(iters=0), dict(iters=65), dict(iters=True), dict(alpha=0.0), dict(alpha=1.0),
               dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha="x"),
               dict(alpha=1 - 1e-12), dict(shortlist=4), dict(shortlist=3001), dict(shortlist=1025), dict(shortlist=100.0),
               dict(shortlist=64, kq=65)):
        with pytest.raises(MI355Error):
            D.diffusion_params(3000, 5, **kw)
    for G, k, kw in ((20, 5, {}), (21, 5, dict(kd=21)), (3000, 1025, {}), (300, 0, {}), (300, True, {}), (300, 8, dict(shortlist=7))):
        with pytest.raises(MI355Error):                                            # kd >= G; L above 1024; k < 1; L < k
            D.diffusion_params(G, k, **kw)
    for kw in (dict(kd=0), dict(kd=33), dict(kd=300), dict(gamma=0), dict(gamma=9)):
        with pytest.raises(MI355Error):
            D.index_params(300, **kw)


def test_python_api_rejects_cpu_tensors():
    q, g = torch.randn(4, 8), torch.randn(40, 8)
    with pytest.raises(MI355Error, match="GPU"):
        M.diffusion_rerank(q, g, 2)
    gal = R.Gallery(8, "cpu")
    with pytest.raises(MI355Error):
        gal.diffuse(q, 2)
    with pytest.raises(MI355Error):
        gal.diffusion_index(20)                                  # kd >= rows
    i64, f32 = torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 3)
    with pytest.raises(MI355Error, match="GPU"):
        D._df_graph(i64, f32, 3)
    with pytest.raises(MI355Error, match="GPU"):
        D._df_source(f32, i64, 2, 3)
    with pytest.raises(MI355Error, match="GPU"):
        D._df_solve(i64.int(), f32, i64, f32, 0.99, 20)


def test_where_the_public_names_live():
    assert "diffuse" not in vars(M.Gallery) and "diffusion_index" not in vars(M.Gallery)
    assert callable(M.Gallery.diffuse) and callable(M.Gallery.diffusion_index)
    assert "DiffusionIndex" not in M.__all__ and "diffusion_rerank" not in M.__all__
    assert M.DiffusionIndex is D.DiffusionIndex and M.diffusion_rerank is D.diffusion_rerank
