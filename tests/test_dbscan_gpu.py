"""``dbscan`` / ``connected_components`` on the GPU against two references: the NumPy model (tests/dbscan_ref.py) fed with the
CSR of the same gallery's own ``range_search`` of its rows - exact, bit for bit, whatever the scores - and the model fed with
float64 scores of the stored rows, valid because the fixtures keep every pair at least 1e-3 from the threshold (asserted
first).  Every result must also be the same bits for every block size, under a forced two-launch tile cut and on a second run:
the union-find's hooks, the border maxima and the degree sums may not depend on any order.

All fixtures have 300 rows (three 128-column tiles, the last of 44) at D = 70 (the exact fp32 loop) and D = 96 (the MFMA loops)."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dbscan_ref as ref
import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["tensor", "strided", "f32", "f16"]
DIMS = [70, 96]
N = ref.N_ROWS


@pytest.fixture(autouse=True)
def _restore_the_override():
    yield
    assert lib().mi355_rank_set_round_slots(0) == 0


def _raw(x):
    """The fixture's unit rows as raw embeddings: each row scaled by 1/2, 1, 2 or 4 - powers of two, so that the normalised
    row has the bits of the fixture's row and the star's tied row keeps equal scores to both cores."""
    return x * (2.0 ** (np.arange(len(x)) % 4 - 1))[:, None].astype(np.float32)


def _rows_of_kind(x, kind):
    """(what dbscan is given, the fp32 / fp16 Gallery whose range search defines its hits)"""
    t = torch.from_numpy(_raw(x)).to(DEV)
    dtype = torch.float16 if kind == "f16" else torch.float32
    gal = M.Gallery(x.shape[1], DEV, dtype=dtype).add(t)
    if kind == "tensor":
        return t, gal
    if kind == "strided":
        big = torch.zeros((len(x), x.shape[1] + 5), device=DEV)
        big[:, : x.shape[1]] = t
        view = big[:, : x.shape[1]]
        assert not view.is_contiguous()
        return view, gal
    return gal, gal


def _csr(gal, t):
    r = gal.range_search(gal.data.float(), t)
    return r.offsets.cpu().numpy(), r.indices.cpu().numpy(), r.scores.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(fixture, dim, kind):
    x = ref.chains(dim)[0] if fixture == "chains" else ref.star(dim)
    t, ms = (ref.CHAIN_T, ref.CHAIN_MIN) if fixture == "chains" else (ref.STAR_T, ref.STAR_MIN)
    rows, gal = _rows_of_kind(x, kind)
    stored = gal.data.float().cpu().numpy()
    return SimpleNamespace(rows=rows, gal=gal, t=t, ms=ms, stored=stored, csr=_csr(gal, t))


def _assert_same(got, want, what=""):
    """A DBSCANResult against a model dict (or another DBSCANResult), exactly."""
    if isinstance(want, M.DBSCANResult):
        want = {f: getattr(want, f).cpu().numpy() for f in ("labels", "core", "degree", "roots", "counts")}
    for f in ("labels", "core", "degree", "roots", "counts"):
        g = getattr(got, f)
        assert g.dtype == (torch.bool if f == "core" else torch.int64) and g.device.type == "cuda", (what, f)
        g = g.cpu().numpy()
        assert g.shape == want[f].shape and (g == want[f]).all(), (what, f, np.flatnonzero(g != want[f])[:8] if g.shape == want[f].shape else g.shape)
    assert got.n_clusters == len(want["roots"]) and got.n_noise == int((want["labels"] < 0).sum()), what


def _tail_tiles():
    out = (C.c_int * 5)()
    assert lib().mi355_rank_last_tiles(out, 5) == 5
    return out[3]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("fixture", ["chains", "star"])
def test_equals_the_model_of_the_gallerys_own_range_search_and_the_float64_model(fixture, dim, kind):
    c = _case(fixture, dim, kind)
    got = M.dbscan(c.rows, c.t, c.ms)
    want = ref.model(N, *c.csr, c.ms)
    _assert_same(got, want, "(a) the model of the range search's CSR")
    margin = ref.margin64(c.stored, c.t)
    print(f"[dbscan] {fixture} D={dim} {kind}: float64 margin {margin:.2e}, nnz {len(c.csr[1])}")
    assert margin >= 1e-3
    _assert_same(got, ref.model64(c.stored, c.t, c.ms), "(b) the float64 model")
    if fixture == "chains":
        assert sorted(got.counts.tolist()) == [140, 150] and int(got.core.sum()) == 286 and got.n_clusters == 2 and got.n_noise == 10
        assert int(((got.labels >= 0) & ~got.core).sum()) == 4
    else:
        assert got.degree.cpu().numpy()[ref.STAR_ROWS].tolist() == ref.STAR_DEGREES
        assert got.labels.cpu().numpy()[ref.STAR_ROWS].tolist() == ref.STAR_LABELS
        assert got.roots.tolist() == [int(ref.STAR_ROWS[0]), int(ref.STAR_ROWS[4])] and got.n_noise == N - 9


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("fixture", ["chains", "star"])
def test_same_bits_for_every_block_tile_cut_and_run(fixture, dim, kind):
    c = _case(fixture, dim, kind)
    want = ref.model(N, *c.csr, c.ms)
    for block in (64, 128, N):
        _assert_same(M.dbscan(c.rows, c.t, c.ms, block=block), want, f"block={block}")
        assert _tail_tiles() == 0
    _assert_same(M.dbscan(c.rows, c.t, c.ms), want, "a second run")
    assert lib().mi355_rank_set_round_slots(4) == 0       # 3 x 3 tiles of 128 queries on 4 slots: 2 column tiles, then a tail launch
    try:
        got = M.dbscan(c.rows, c.t, c.ms, block=N)
        assert _tail_tiles() > 0
    finally:
        assert lib().mi355_rank_set_round_slots(0) == 0
    _assert_same(got, want, "a main launch of 128-query tiles and a tail launch of 64-query tiles")


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("t", [0.9, 0.5, -1.0])
def test_dense_graphs_equal_the_model(t, dim, kind):
    """Lower thresholds on the chains: tens to hundreds of hits per row, down to every pair a hit (one component of 300 rows,
    every hook contended).  No margin is needed: the model reads the hits of the gallery's own range search."""
    c = _case("chains", dim, kind)
    csr = _csr(c.gal, t)
    for ms in (1, 5, 40):
        want = ref.model(N, *csr, ms)
        for block in (128, N):
            _assert_same(M.dbscan(c.rows, t, ms, block=block), want, f"t={t} min_samples={ms} block={block}")
    if t == -1.0:
        got = M.connected_components(c.rows, t)
        assert got.n_clusters == 1 and got.counts.tolist() == [N] and got.roots.tolist() == [0] and got.degree.tolist() == [N] * N


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_min_samples_one_is_connected_components_and_a_large_one_is_all_noise(dim, kind):
    c = _case("chains", dim, kind)
    comp = M.connected_components(c.rows, c.t)
    _assert_same(comp, ref.model(N, *c.csr, 1), "components")
    _assert_same(M.dbscan(c.rows, c.t, 1), comp, "dbscan(min_samples=1)")
    assert comp.core.all() and comp.n_noise == 0 and comp.n_clusters == 12 and sorted(comp.counts.tolist())[-2:] == [140, 150]
    top = int(comp.degree.max())
    for ms in (top + 1, N + 1, 1 << 40):
        noise = M.dbscan(c.rows, c.t, ms)
        assert noise.n_clusters == 0 and noise.n_noise == N and (noise.labels == -1).all() and not noise.core.any()
        assert noise.roots.shape == noise.counts.shape == (0,) and torch.equal(noise.degree, comp.degree)
    _assert_same(M.dbscan(c.rows, c.t, top), ref.model(N, *c.csr, top), "min_samples = the largest degree")


@pytest.mark.parametrize("kind", ["tensor", "f32", "f16"])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", [1, 129])
def test_one_row_and_one_row_past_a_tile(n, dim, kind):
    x = ref.chains(dim)[0][:n]
    rows, gal = _rows_of_kind(x, kind)
    for t in (ref.CHAIN_T, 0.5):
        csr = _csr(gal, t)
        for ms in (1, 2, 3):
            _assert_same(M.dbscan(rows, t, ms), ref.model(n, *csr, ms), f"n={n} t={t} min_samples={ms}")
    if n == 1:
        one = M.dbscan(rows, 0.5, 1)
        assert one.labels.tolist() == [0] and one.degree.tolist() == [1] and one.roots.tolist() == [0] and one.n_noise == 0
        assert M.dbscan(rows, 0.5, 2).labels.tolist() == [-1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_gallery_methods(dtype):
    c = _case("chains", 96, "f16" if dtype == torch.float16 else "f32")
    want = ref.model(N, *c.csr, c.ms)
    _assert_same(c.gal.dbscan(c.t, c.ms), want, "Gallery.dbscan")
    _assert_same(c.gal.dbscan(c.t, c.ms, block=100), want, "Gallery.dbscan(block=100)")
    _assert_same(c.gal.components(c.t), ref.model(N, *c.csr, 1), "Gallery.components")
    if dtype == torch.float32:                            # a prepared gallery is clustered on its fp32 rows
        g = M.Gallery(96, DEV).add(c.gal.data).prepare()
        _assert_same(g.dbscan(c.t, c.ms), ref.model(N, *_csr(g, c.t), c.ms), "a prepared gallery")
    empty = M.Gallery(96, DEV, dtype=dtype).dbscan(0.5, 2)
    assert empty.n_clusters == 0 and empty.n_noise == 0 and empty.labels.shape == (0,)
    scores = M.clustering_metrics(M.dbscan(c.gal, c.t, c.ms).labels, torch.from_numpy(ref.chains(96)[1]).to(DEV))
    assert scores["n_clusters"] == 3 and scores["n_classes"] == 3          # the noise rows, label -1, count as one cluster


# ---------------------------------------------------------------- many workgroups on one union-find
BIG_N = 4096 + 37                    # 33 x 33 tiles of 128 queries in one GEMM call: every CU hooks into the same parent[]


@functools.lru_cache(maxsize=None)
def _planted(dim=96, centres=30):
    rng = np.random.default_rng(5)
    c = rng.standard_normal((centres, dim))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    lab = rng.permutation(BIG_N) % centres                # a cluster's rows lie in every tile
    x = c[lab] + 0.03 * rng.standard_normal((BIG_N, dim))
    return x.astype(np.float32), lab


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_one_component_of_every_row_hooked_by_a_thousand_workgroups(dtype):
    """t = -1: all 17 million pairs are hits between core rows, so every workgroup of the link pass unions into ONE component
    at once.  The result is known without a model: root 0, every degree N; and it is the same for two block sizes."""
    gal = M.Gallery(96, DEV, dtype=dtype).add(torch.from_numpy(_planted()[0]).to(DEV))
    for block in (None, 1000):
        got = gal.components(-1.0, block=block)
        assert got.n_clusters == 1 and got.n_noise == 0 and got.roots.tolist() == [0] and got.counts.tolist() == [BIG_N]
        assert (got.labels == 0).all() and got.core.all() and (got.degree == BIG_N).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_planted_clusters_spread_over_every_tile_equal_the_model(dtype):
    """30 tight clusters of ~138 rows whose members lie in all 33 column tiles (scores of at least 0.83 inside a cluster, at most 0.46
    between two, against t = 0.8): about 570 000 hits, every union between rows of different workgroups.  Against the model of the gallery's own range
    search, and - the clusters being the planted ones - against the planted labels."""
    x, lab = _planted()
    gal = M.Gallery(96, DEV, dtype=dtype).add(torch.from_numpy(x).to(DEV))
    csr = _csr(gal, 0.8)
    want = ref.model(BIG_N, *csr, 5)
    _assert_same(gal.dbscan(0.8, 5), want, "block = 4096")
    _assert_same(gal.dbscan(0.8, 5, block=1000), want, "block = 1000: query blocks that start inside a tile")
    assert want["labels"].min() == 0 and len(want["roots"]) == 30
    assert len(set(zip(want["labels"].tolist(), lab.tolist()))) == 30
