"""Result diversification without a GPU: the new symbols are declared, bound and exported; every guard of mi355_shortlist_gram and
mi355_mmr_select (rejected before any HIP call, with a message) and of the Python API; and where the public names live."""
import ctypes
import math

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib, diversify as D
from imageretrievalresearch_amd import rank as R

NAMES = ["mi355_shortlist_gram", "mi355_mmr_select"]
F32, F16 = _lib.DTYPE_F32, _lib.DTYPE_F16


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_are_declared_bound_and_exported():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert _lib.lib().mi355_abi_version() == 3


def _gram(rows=16, dtype=F32, ld=64, G=100, dim=64, idx=8, Q=4, L=64, out=4):
    return _lib.lib().mi355_shortlist_gram(rows, dtype, ld, G, dim, idx, Q, L, out, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(rows=None), b"null"), (dict(idx=None), b"null"), (dict(out=None), b"null"), (dict(dtype=7), b"dtype 7"),
    (dict(G=0), b"G=0"), (dict(G=1 << 31), b"G="), (dict(dim=0), b"dim=0"), (dict(dim=65537, ld=65537), b"dim=65537"),
    (dict(ld=63), b"ld=63"), (dict(ld=1 << 31), b"ld="), (dict(Q=-1), b"Q=-1"), (dict(Q=1 << 31), b"Q="), (dict(L=0), b"L=0"),
    (dict(L=1025), b"L=1025"), (dict(dtype=F16, ld=68), b"multiple of 8"), (dict(dtype=F16, rows=8), b"16-byte"),
    (dict(rows=2), b"4-byte"), (dict(idx=4), b"8-byte"), (dict(out=2), b"4-byte"),
])
def test_gram_entry_rejects_bad_arguments(kw, msg):
    assert _gram(**kw) != 0
    assert msg in _err(), (kw, _err())


def _select(rel=4, idx=8, gram=4, Q=4, L=64, k=10, lam=0.7, dedup=math.nan, off=0, val=4, out_idx=8, mmr=None, count=None):
    return _lib.lib().mi355_mmr_select(rel, idx, gram, Q, L, k, lam, dedup, off, val, out_idx, mmr, count, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(rel=None), b"null"), (dict(idx=None), b"null"), (dict(gram=None), b"null"), (dict(val=None), b"null"),
    (dict(out_idx=None), b"null"), (dict(Q=-1), b"Q=-1"), (dict(Q=1 << 31), b"Q="), (dict(L=0), b"L=0"), (dict(L=1025), b"L=1025"),
    (dict(k=0), b"k=0"), (dict(k=65), b"k=65"), (dict(lam=-0.1), b"lam"), (dict(lam=1.5), b"lam"), (dict(lam=math.nan), b"lam"),
    (dict(lam=math.inf), b"lam"), (dict(dedup=math.inf), b"dedup"), (dict(dedup=-math.inf), b"dedup"), (dict(idx=4), b"8-byte"),
    (dict(out_idx=4), b"8-byte"),
])
def test_select_entry_rejects_bad_arguments(kw, msg):
    assert _select(**kw) != 0
    assert msg in _err(), (kw, _err())


def test_zero_queries_do_nothing():
    assert _gram(Q=0) == 0 and _gram(Q=0, dtype=F16, L=1024, dim=1, ld=8) == 0
    assert _select(Q=0) == 0 and _select(Q=0, L=1024, k=1024, lam=0.0, dedup=0.5) == 0 and _select(Q=0, L=1, k=1, lam=1.0) == 0


def test_python_parameters():
    assert D.diversify_params(3000, 10) == (10, 0.7, None, 100, 6710)              # 256 MiB of 100 x 100 fp32 matrices
    assert D.diversify_params(3000, 5) == (5, 0.7, None, 100, 6710)                # shortlist default: max(10 k, 100) ...
    assert D.diversify_params(3000, 30)[3] == 300
    assert D.diversify_params(3000, 500)[3] == 1024                                # ... capped at 1024 ...
    assert D.diversify_params(150, 20)[3] == 150                                   # ... and at the rows
    assert D.diversify_params(3000, 10, shortlist=1024)[3:] == (1024, 64)
    assert D.diversify_params(3000, 10, lam=0, dedup=0.95, shortlist=10, block=8) == (10, 0.0, 0.95, 10, 8)
    assert D.diversify_params(3000, 10, lam=1, dedup=-2)[1:3] == (1.0, -2.0)
    for kw in (dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam="x"), dict(lam=None),
               dict(dedup=float("nan")), dict(dedup=float("inf")), dict(dedup=1e300), dict(dedup="x"), dict(dedup=True),
               dict(shortlist=9), dict(shortlist=3001), dict(shortlist=1025), dict(shortlist=100.0), dict(shortlist=True),
               dict(block=0), dict(block=-1), dict(block=2.0), dict(block=True)):
        with pytest.raises(MI355Error):
            D.diversify_params(3000, 10, **kw)
    for G, k in ((3000, 0), (3000, True), (3000, 2.0), (3000, 1025), (5, 6)):
        with pytest.raises(MI355Error):
            D.diversify_params(G, k)


def test_python_api_rejects_cpu_tensors_and_other_galleries():
    q, g = torch.randn(4, 8), torch.randn(40, 8)
    with pytest.raises(MI355Error, match="GPU"):
        M.mmr_rerank(q, g, 2)
    gal = R.Gallery(8, "cpu")
    with pytest.raises(MI355Error):
        gal.diversify(q, 2)
    i64, f32 = torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 3)
    with pytest.raises(MI355Error, match="GPU"):
        D._dv_gram(gal, i64)
    with pytest.raises(MI355Error, match="GPU"):
        D._dv_select(f32, i64, torch.zeros(4, 3, 3), 2, 0.7, None)
    for other in (M.Int8Gallery(8, "cpu"), object()):
        with pytest.raises(MI355Error, match="not supported"):
            D.diversify(other, q, 2)
        with pytest.raises(MI355Error, match="not supported"):
            D._dv_gram(other, i64)
    assert not hasattr(M.Int8Gallery, "diversify") and not hasattr(M.ShardedGallery, "diversify")


def test_where_the_public_names_live():
    assert "diversify" not in vars(M.Gallery) and callable(M.Gallery.diversify)
    assert "mmr_rerank" not in M.__all__ and M.mmr_rerank is D.mmr_rerank
    assert R._Diversified in M.Gallery.__bases__
