"""The k-means / clustering entries without a GPU: the ABI names, every argument error before any HIP call, workspace sizes
of empty inputs, the host-side scores against the float64 reference, and the Python argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import kmeans_ref as ref
from helpers import header_symbols
from imageretrievalresearch_amd import _lib

NEW = ["mi355_nearest_centroid", "mi355_nearest_centroid_workspace_bytes", "mi355_nearest_centroid_f16",
       "mi355_nearest_centroid_f16_workspace_bytes", "mi355_cluster_members", "mi355_cluster_members_workspace_bytes",
       "mi355_centroid_update", "mi355_centroid_update_f16", "mi355_centroid_update_workspace_bytes",
       "mi355_centroid_update_f16_workspace_bytes", "mi355_contingency", "mi355_contingency_workspace_bytes"]
P = 0x1000        # a non-null, 16-byte aligned address that no check may dereference


def test_new_entries_are_declared_bound_and_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name
    assert _lib.lib().mi355_abi_version() == 3


def _fails(status, word):
    msg = _lib.lib().mi355_last_error()
    assert status != 0 and word.encode() in msg, (status, msg)


def test_nearest_centroid_argument_errors():
    L = _lib.lib()
    for f16 in (False, True):
        def call(c=P, K=4, r=P, N=10, dim=8, qb=0, a=P, s=P, ws=P, wsb=1 << 30):
            if f16:
                return L.mi355_nearest_centroid_f16(c, K, r, N, dim, 1e-6, qb, a, s, ws, wsb, None)
            return L.mi355_nearest_centroid(c, K, r, N, dim, 0, 1e-6, qb, a, s, ws, wsb, None)
        _fails(call(c=None), "null")
        _fails(call(r=None), "null")
        _fails(call(a=None), "null")
        _fails(call(s=None), "null")
        _fails(call(K=0), "bad shape")
        _fails(call(N=0), "bad shape")
        _fails(call(dim=0), "bad shape")
        _fails(call(N=1 << 31), "too large")
        _fails(call(qb=-1), "query_block")
        _fails(call(ws=None), "workspace")
        _fails(call(wsb=16), "workspace")
    _fails(L.mi355_nearest_centroid_f16(P, 4, P + 8, 10, 8, 1e-6, 0, P, P, P, 1 << 30, None), "16-byte aligned")


def test_members_and_update_argument_errors():
    L = _lib.lib()
    _fails(L.mi355_cluster_members(None, 10, 3, P, P, P, 1 << 20, None), "null")
    _fails(L.mi355_cluster_members(P, 10, 3, None, P, P, 1 << 20, None), "null")
    _fails(L.mi355_cluster_members(P, 10, 3, P, None, P, 1 << 20, None), "null")
    _fails(L.mi355_cluster_members(P, 0, 3, P, P, P, 1 << 20, None), "N=")
    _fails(L.mi355_cluster_members(P, 10, 0, P, P, P, 1 << 20, None), "n_clusters")
    # one workgroup of 256 threads per cluster: 2^24 of them would pass the 2^32 threads of a grid dimension
    _fails(L.mi355_cluster_members(P, 1 << 25, 1 << 24, P, P, P, 1 << 40, None), "n_clusters")
    _fails(L.mi355_cluster_members(P, 10, 3, P, P, None, 0, None), "workspace")
    _fails(L.mi355_cluster_members(P, 10, 3, P, P, P, 8, None), "workspace")
    for fn in (L.mi355_centroid_update, L.mi355_centroid_update_f16):
        def call(r=P, N=10, dim=8, a=P, K=3, prev=P, out=P, cnt=P, off=P, order=P, ws=P, wsb=1 << 30):
            return fn(r, N, dim, a, K, prev, 1e-6, out, cnt, off, order, ws, wsb, None)
        for kw in ("r", "a", "prev", "out", "cnt", "off", "order"):
            _fails(call(**{kw: None}), "null")
        _fails(call(N=0), "N=")
        _fails(call(K=0), "n_clusters")
        _fails(call(dim=0), "dim=")
        _fails(call(K=1 << 24, N=1 << 25), "n_clusters")
        _fails(call(N=((1 << 24) - 1) * 256 + 1), "too large")                 # more rows than 2^24 - 1 segments hold
        _fails(call(N=((1 << 24) - 4) * 256, K=4), "too large")                # segments of the rows + one spare per cluster
        _fails(call(N=1 << 62, K=5), "too large")
        _fails(call(ws=None), "workspace")
        _fails(call(wsb=64), "workspace")
    _fails(L.mi355_centroid_update_f16(P + 2, 10, 8, P, 3, P, 1e-6, P, P, P, P, P, 1 << 30, None), "16-byte aligned")


def test_contingency_argument_errors():
    L = _lib.lib()
    _fails(L.mi355_contingency(None, P, 5, 2, 2, P, P, 1024, None), "null")
    _fails(L.mi355_contingency(P, None, 5, 2, 2, P, P, 1024, None), "null")
    _fails(L.mi355_contingency(P, P, 5, 2, 2, None, P, 1024, None), "null")
    _fails(L.mi355_contingency(P, P, 0, 2, 2, P, P, 1024, None), "N=")
    _fails(L.mi355_contingency(P, P, (1 << 40) + 1, 2, 2, P, P, 1024, None), "N=")
    _fails(L.mi355_contingency(P, P, 5, 0, 2, P, P, 1024, None), "must be >= 1")
    _fails(L.mi355_contingency(P, P, 5, 1 << 20, 1 << 20, P, P, 1024, None), "too large")
    _fails(L.mi355_contingency(P, P, 5, 1 << 40, 1 << 40, P, P, 1024, None), "too large")
    _fails(L.mi355_contingency(P, P, 5, 2, 2, P, None, 0, None), "workspace")
    _fails(L.mi355_contingency(P, P, 5, 2, 2, P, P, 4, None), "workspace")


def test_workspace_sizes():
    L = _lib.lib()
    assert L.mi355_nearest_centroid_workspace_bytes(0, 10, 8) == 0 and L.mi355_nearest_centroid_workspace_bytes(4, 0, 8) == 0
    assert L.mi355_nearest_centroid_f16_workspace_bytes(0, 10, 8) == 0 and L.mi355_nearest_centroid_f16_workspace_bytes(4, 0, 8) == 0
    assert L.mi355_cluster_members_workspace_bytes(0, 3) == 0 and L.mi355_cluster_members_workspace_bytes(10, 0) == 0
    assert L.mi355_centroid_update_workspace_bytes(0, 3, 8) == 0 and L.mi355_centroid_update_workspace_bytes(10, 3, 0) == 0
    assert L.mi355_centroid_update_f16_workspace_bytes(0, 3, 8) == 0 and L.mi355_centroid_update_f16_workspace_bytes(10, 3, 0) == 0
    assert L.mi355_centroid_update_f16_workspace_bytes(1000, 7, 70) == L.mi355_centroid_update_workspace_bytes(1000, 7, 70) > 0
    assert L.mi355_contingency_workspace_bytes(0, 2, 2) == 0
    # no N x K score slab and no candidate lists: 8 B per row, the centroids and their planes, 4 B per row for the norms
    assert L.mi355_nearest_centroid_workspace_bytes(1000, 100000, 1536) < 24 * 2**20
    assert L.mi355_nearest_centroid_f16_workspace_bytes(1000, 100000, 1536) < L.mi355_nearest_centroid_workspace_bytes(1000, 100000, 1536)
    # the partial sums: (N / 256 + K) segments of dim float64
    assert L.mi355_centroid_update_workspace_bytes(100000, 1000, 1536) < (100000 // 256 + 1002) * 1536 * 8 + 2**16


def test_metrics_from_table_match_the_reference():
    rng = np.random.default_rng(5)
    tables = [rng.integers(0, 9, (7, 4)), np.array([[3, 1], [0, 4]]), np.array([[5]]), np.eye(6, dtype=np.int64) * 3,
              np.outer([2, 3, 5], [1, 4]), np.array([[1], [1], [1]]), rng.integers(0, 4000, (40, 55))]
    for t in tables:
        got, want = M.clustering_metrics_from_table(t), ref.metrics_from_table(t)
        for k in ("nmi", "purity", "f1", "precision", "recall"):
            assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k], t.shape)
        assert got["n_clusters"] == want["n_clusters"] and got["n_classes"] == want["n_classes"]
    assert M.clustering_metrics_from_table(torch.tensor([[2, 0], [0, 2]]))["nmi"] == pytest.approx(1.0, abs=1e-15)
    for bad in (np.zeros((2, 2), np.int64), np.array([1, 2]), np.array([[1.5]]), np.array([[-1, 2]])):
        with pytest.raises(M.MI355Error):
            M.clustering_metrics_from_table(bad)


def test_python_argument_checks_need_no_gpu():
    x, c = torch.zeros(6, 4), torch.ones(2, 4)
    for call in (lambda: M.assign_clusters(x, c), lambda: M.spherical_kmeans(x, 2), lambda: M.spherical_kmeans(x, 2, init=c),
                 lambda: M.update_centroids(x, torch.zeros(6, dtype=torch.int64), 2, c),
                 lambda: M.contingency(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)),
                 lambda: M.clustering_metrics(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(M.MI355Error, match="GPU"):
            call()
    with pytest.raises(M.MI355Error):
        M.assign_clusters("rows", c)
    with pytest.raises(M.MI355Error):
        M.assign_clusters(x, None)


def test_shape_checks_come_before_any_launch(monkeypatch):
    # pretend the tensors are on the GPU: every call below must raise on its shapes before it reaches the library
    from imageretrievalresearch_amd import cluster, rank
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)
    monkeypatch.setattr(cluster, "require_cuda", lambda t, name: None)
    monkeypatch.setattr(cluster, "lib", lambda: pytest.fail("reached the library"))
    x = torch.zeros(6, 4)
    with pytest.raises(M.MI355Error, match="dims differ"):
        M.assign_clusters(x, torch.ones(2, 5))
    with pytest.raises(M.MI355Error, match="K >= 1"):
        M.assign_clusters(x, torch.ones(4))
    with pytest.raises(M.MI355Error, match="K >= 1"):
        M.assign_clusters(x, torch.ones(0, 4))
    with pytest.raises(M.MI355Error, match="block"):
        M.assign_clusters(x, torch.ones(2, 4), block=0)
    with pytest.raises(M.MI355Error):
        M.assign_clusters(torch.zeros(6), torch.ones(2, 4))
    for k in (0, 7, -1, 2.0, True):
        with pytest.raises(M.MI355Error, match="n_clusters"):
            M.spherical_kmeans(x, k)
    with pytest.raises(M.MI355Error, match="init"):
        M.spherical_kmeans(x, 2, init=torch.ones(3, 4))
    with pytest.raises(M.MI355Error, match="dims differ"):
        M.spherical_kmeans(x, 2, init=torch.ones(2, 3))
    with pytest.raises(M.MI355Error, match="iters"):
        M.spherical_kmeans(x, 2, iters=-1)
    with pytest.raises(M.MI355Error, match="assign"):
        M.update_centroids(x, torch.zeros(5, dtype=torch.int64), 2, torch.ones(2, 4))
    with pytest.raises(M.MI355Error, match="previous"):
        M.update_centroids(x, torch.zeros(6, dtype=torch.int64), 2, torch.ones(3, 4))
    with pytest.raises(M.MI355Error, match="integers"):
        M.contingency(torch.zeros(3), torch.zeros(3, dtype=torch.int64))


def test_seeded_rows_are_distinct_and_portable():
    from imageretrievalresearch_amd.cluster import seeded_rows
    a, b = seeded_rows(1000, 50, 3), seeded_rows(1000, 50, 3)
    assert (a == b).all() and len(set(a.tolist())) == 50 and a.min() >= 0 and a.max() < 1000
    assert (seeded_rows(1000, 50, 4) != a).any()
    assert seeded_rows(5, 5, 0).tolist() == np.argsort(M.synth.uniform(0, (5,)), kind="stable").tolist()


def test_gallery_clustering_metrics_needs_labels():
    g = M.Gallery.__new__(M.Gallery)
    g.labels, g.rows = None, 3
    with pytest.raises(M.MI355Error, match="labels"):
        g.clustering_metrics()
