"""Regional MaxSim re-ranking without a GPU: the new symbols are declared, bound and exported; every guard of mi355_region_scores
(rejected before any HIP call, with a message) and of the Python API; the LDS sizer; and where the public names live."""
import ctypes

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib, regional as RG
from imageretrievalresearch_amd import rank as R

NAMES = ["mi355_region_scores", "mi355_region_scores_lds_bytes"]


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_are_declared_bound_and_exported():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert _lib.lib().mi355_abi_version() == 3


def _scores(qc=16, Q=4, Rq=14, gc=16, rows=100, R=14, dim=128, ld=128, idx=16, L=50, w=None, out=16, mt=None):
    return _lib.lib().mi355_region_scores(qc, Q, Rq, gc, rows, R, dim, ld, idx, L, w, out, mt, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(qc=None), b"null"), (dict(gc=None), b"null"), (dict(out=None), b"null"), (dict(Q=-1), b"Q=-1"), (dict(Q=1 << 31), b"Q="),
    (dict(Rq=0), b"Rq=0"), (dict(Rq=65), b"Rq=65"), (dict(R=0), b"R=0"), (dict(R=65), b"R=65"), (dict(rows=0), b"rows=0"),
    (dict(rows=1 << 31), b"rows="), (dict(dim=0), b"dim=0"), (dict(dim=65537, ld=65600), b"dim=65537"), (dict(ld=120), b"ld=120"),
    (dict(ld=192), b"ld=192"), (dict(dim=130, ld=128), b"ld=128"), (dict(L=0), b"L=0"), (dict(L=1025), b"L=1025"),
    (dict(idx=None, L=50), b"L=50"), (dict(qc=8), b"aligned"), (dict(gc=24), b"aligned"),
])
def test_entry_rejects_bad_arguments(kw, msg):
    assert _scores(**kw) != 0
    assert msg in _err(), (kw, _err())


def test_zero_queries_do_nothing():
    assert _scores(Q=0) == 0 and _scores(Q=0, idx=None, L=100) == 0


def test_lds_sizer():
    size = _lib.lib().mi355_region_scores_lds_bytes
    cap = 64 * 1024
    assert size(14, 1536) == 16 * (1536 + 8) * 2                # resident: 16 padded rows of ld + 8 halfs
    assert size(14, 1500) == size(16, 1536) == size(1, 1473)    # Rq to the 16-row tile, dim to the 128-byte segment
    assert size(1, 1) == 16 * (64 + 8) * 2
    assert size(17, 200) == 32 * (256 + 8) * 2
    for Rq, dim in ((64, 2560), (64, 1536), (32, 1536), (16, 2048), (64, 65536), (14, 65536)):
        need = size(Rq, dim)                                     # chunks of d: whole segments, as many as fit the cap
        rows = (Rq + 15) // 16 * 16
        chunk = need // (rows * 2) - 8
        assert 0 < need <= cap and chunk >= 64 and chunk % 64 == 0 and rows * (chunk + 64 + 8) * 2 > cap, (Rq, dim, need)
    assert RG.lds_bytes(14, 1536) == size(14, 1536) and RG.LDS_BYTES == cap
    for Rq, dim in ((0, 128), (65, 128), (14, 0), (14, 65537), (-1, -1)):
        assert size(Rq, dim) == 0, (Rq, dim)


def test_constructor_and_parameters():
    rg = M.RegionGallery(70, 14, "cpu", capacity=5)
    assert (rg.dim, rg.regions, len(rg), rg.nbytes) == (70, 14, 0, 5 * 14 * 128 * 2)
    assert tuple(rg.data.shape) == (0, 14, 70) and rg._buf.dtype == torch.float16 and rg.labels is None
    for kw in (dict(regions=0), dict(regions=65), dict(regions=2.0), dict(regions=True), dict(dim=0), dict(dim=65537)):
        with pytest.raises(MI355Error):
            M.RegionGallery(**{**dict(dim=8, regions=3, device="cpu"), **kw})
    assert RG.rerank_params(3000, 5) == (5, 100) and RG.rerank_params(40, 5) == (5, 40) and RG.rerank_params(3000, 250) == (250, 250)
    assert RG.rerank_params(3000, 1, 1024) == (1, 1024) and RG.rerank_params(7, 7, 7) == (7, 7)
    for rows, k, sl in ((3000, 0, None), (3000, True, None), (3000, 2.0, None), (3000, 1025, None), (3000, 5, 4), (3000, 5, 1025),
                        (3000, 5, 100.0), (50, 5, 51), (50, 51, None)):
        with pytest.raises(MI355Error):
            RG.rerank_params(rows, k, sl)


def _rg(rows=6, dim=8, regions=3):
    rg = M.RegionGallery(dim, regions, "cpu", capacity=rows)
    rg.rows = rows                                               # argument checks only: nothing is launched on these rows
    return rg


@pytest.mark.parametrize("bad, match", [
    (lambda rg: rg.add(torch.zeros(2, 8)), "regions must be"),                                  # rank
    (lambda rg: rg.add(torch.zeros(2, 3, 9)), "regions must be"),                               # dim
    (lambda rg: rg.add(torch.zeros(2, 4, 8)), "3 regions"),                                     # another R
    (lambda rg: rg.add(torch.zeros(2, 3, 8, dtype=torch.int32)), "float"),                      # dtype
    (lambda rg: rg.add(torch.zeros(2, 3, 8, dtype=torch.float64)), "float"),
    (lambda rg: rg.add([[1.0]]), "tensor"),
    (lambda rg: rg.add(torch.zeros(2, 3, 8)), "GPU"),                                           # device
    (lambda rg: rg.query_codes(torch.zeros(8)), "query_regions must be"),
    (lambda rg: rg.query_codes(torch.zeros(2, 0, 8)), "outside"),                               # Rq = 0
    (lambda rg: rg.query_codes(torch.zeros(2, 65, 8)), "outside"),                              # Rq = 65
    (lambda rg: rg.query_codes(torch.zeros(2, 5, 8)), "GPU"),
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), torch.zeros(2, 4)), "int64"),                   # idx dtype
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), torch.zeros(2, 4, dtype=torch.int32)), "int64"),
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), torch.zeros(3, 4, dtype=torch.int64)), "idx must be"),   # another Q
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), torch.zeros(8, dtype=torch.int64)), "idx must be"),      # rank
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), torch.zeros(2, 0, dtype=torch.int64)), "L=0"),
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), torch.zeros(2, 1025, dtype=torch.int64)), "L=1025"),
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), weights=torch.zeros(2, 4)), "weights must be"),          # shape
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), weights=torch.zeros(2, 5, dtype=torch.float64)), "weights must be"),
    (lambda rg: rg.scores(torch.zeros(2, 5, 8), weights=[0.2] * 5), "tensor"),
    (lambda rg: rg.scores(torch.zeros(2, 5, 9)), "query_regions must be"),
    (lambda rg: rg.scores(torch.zeros(2, 5, 8)), "GPU"),
    (lambda rg: rg.search(torch.zeros(2, 5, 8), 0), "k=0"),
    (lambda rg: rg.search(torch.zeros(2, 5, 8), 7), "k=7"),
    (lambda rg: rg.search(torch.zeros(2, 5, 8), 2.0), "k=2.0"),
    (lambda rg: rg.search(torch.zeros(2, 5, 8), 2), "GPU"),
    (lambda rg: rg.rerank(torch.zeros(6, 8), torch.zeros(2, 8), torch.zeros(2, 5, 8), 2), "Gallery"),
    (lambda rg: rg.rerank(R.Gallery(8, "cpu"), torch.zeros(2, 8), torch.zeros(2, 5, 8), 2), "holds 0 rows"),
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 4), torch.zeros(2, 5, 8), 0), "k=0"),
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 4), torch.zeros(2, 5, 8), 7), "shortlist"),
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 4), torch.zeros(2, 5, 8), 3, shortlist=2), "shortlist"),
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 4), torch.zeros(2, 5, 8), 3, shortlist=7), "shortlist"),
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 8), torch.zeros(2, 5, 8), 3), "queries must be"),   # not the gallery's dim
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 4), torch.zeros(3, 5, 8), 3), "query_regions must be"),
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 4), torch.zeros(2, 5, 8), 3, weights=torch.zeros(2, 4)), "weights must be"),
    (lambda rg: rg.rerank(_gal(6, 4), torch.zeros(2, 4), torch.zeros(2, 5, 8), 3), "GPU"),
    (lambda rg: M.maxsim(torch.zeros(2, 5, 8), torch.zeros(6, 8)), "gallery_regions"),
    (lambda rg: M.maxsim(torch.zeros(2, 5, 8), torch.zeros(6, 3, 8)), "GPU"),
])
def test_python_api_rejects_bad_arguments_before_any_launch(bad, match):
    with pytest.raises(MI355Error, match=match):
        bad(_rg())


def _gal(rows, dim):
    g = R.Gallery(dim, "cpu", capacity=rows)
    g.rows = rows
    return g


def test_a_gallery_on_another_device_is_rejected():
    rg = _rg()
    g = _gal(6, 4)
    g.device = torch.device("cuda:0")
    with pytest.raises(MI355Error, match="is on cuda:0"):
        rg.rerank(g, torch.zeros(2, 4), torch.zeros(2, 5, 8), 3)


def test_an_empty_gallery_cannot_be_scored():
    with pytest.raises(MI355Error):
        _rg(rows=0).search(torch.zeros(2, 5, 8), 1)


def test_where_the_public_names_live():
    assert "RegionGallery" not in M.__all__ and "maxsim" not in M.__all__
    assert M.RegionGallery is RG.RegionGallery and M.maxsim is RG.maxsim
    for cls in (M.Gallery, M.Int8Gallery, M.PreparedGallery, M.IVFIndex, M.RerankIndex, M.Whitening):
        assert not [n for n in vars(cls) if "region" in n.lower() or "maxsim" in n.lower()], cls
    assert issubclass(RG.RegionGallery, R._RowStore)
    for name in ("add", "data", "nbytes", "query_codes", "scores", "search", "rerank", "pooled"):
        assert name in vars(RG.RegionGallery), name
