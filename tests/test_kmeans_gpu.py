"""Spherical k-means on the GPU against the float64 reference (tests/kmeans_ref.py): the nearest-centroid epilogue at every
tile edge, the tie rule, the CSR members, the float64 centroid update, the loop on the certified planted inputs, the
contingency table and the clustering scores."""
import functools

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import kmeans_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["f32", "strided", "gallery32", "f16"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).numpy()


def _same_bits(a, b):
    return a.shape == b.shape and (_bits(a) == _bits(b)).all()


@functools.lru_cache(maxsize=None)
def _gauss(seed, N, D):
    return np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32) * 1.7


def _rows(kind, x):
    """(what the call takes, the float64 rows the reference takes, unit_rows): raw fp32 rows (contiguous / strided,
    unnormalised) are normalised by the reference itself; a gallery's stored rows (fp32 / fp16) are taken as they are."""
    t = torch.from_numpy(x).to(DEV)
    if kind == "f32":
        return t, x.astype(np.float64), False
    if kind == "strided":
        buf = torch.full((x.shape[0], x.shape[1] + 3), 7.0, device=DEV)
        buf[:, : x.shape[1]] = t
        v = buf[:, : x.shape[1]]
        assert x.shape[0] == 1 or not v.is_contiguous()
        return v, x.astype(np.float64), False
    g = M.Gallery(x.shape[1], DEV, dtype=torch.float16 if kind == "f16" else torch.float32).add(t)
    return g, g.data.float().cpu().numpy().astype(np.float64), True


def _check_assign(a, s, s64):
    """The score conditions of every row, none left out; returns the rows whose float64 gap certifies the index."""
    a, s = a.cpu().numpy(), s.cpu().numpy().astype(np.float64)
    n = np.arange(s64.shape[0])
    assert a.dtype == np.int64 and a.min() >= 0 and a.max() < s64.shape[1]
    chosen = s64[n, a]
    worst = float((s64.max(axis=1) - chosen).max())
    err = float(np.abs(s - chosen).max())
    print(f"max (f64 best - f64 chosen) {worst:.3e}, max |score - f64 chosen| {err:.3e}")
    assert worst <= 2e-5
    assert err <= 1e-5
    ra, _, gap = _ref_from_scores(s64)
    cert = gap >= 1e-4
    assert (a[cert] == ra[cert]).all()
    return cert


def _ref_from_scores(s64):
    a = s64.argmax(axis=1)
    best = s64[np.arange(s64.shape[0]), a]
    if s64.shape[1] == 1:
        return a, best, np.full(s64.shape[0], np.inf)
    t = s64.copy()
    t[np.arange(s64.shape[0]), a] = -np.inf
    return a, best, best - t.max(axis=1)


# (N, K, D): the 128-column tile edge and a ragged last tile; the 64- and 128-query tile edges (K = 300 is three 128-query
# tiles, 33 x 3 tiles in ONE launch: the two-launch tail needs more tiles than resident workgroups and is reached with forced
# slots in tests/test_rank_tiles_gpu.py); dim % 4, k-step tails and the workload's width
SHAPES = [(1, 1, 1), (127, 2, 7), (128, 63, 64), (129, 64, 70), (4099, 65, 64), (129, 129, 7), (4099, 300, 70),
          (127, 300, 1536), (1, 300, 64), (4099, 7, 1536), (128, 1, 70), (129, 2, 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,K,D", SHAPES)
def test_assign_against_float64(N, K, D, kind):
    x, c = _gauss(1, N, D), _gauss(2, K, D)
    rows, x64, unit = _rows(kind, x)
    s64 = ref.scores(x64, c, unit_rows=unit)
    ct = torch.from_numpy(c).to(DEV)
    a, s = M.assign_clusters(rows, ct)
    assert a.shape == (N,) and s.shape == (N,) and a.dtype == torch.int64 and s.dtype == torch.float32
    _check_assign(a, s, s64)
    a2, s2 = M.assign_clusters(rows, ct)
    assert _same_bits(a, a2) and _same_bits(s, s2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("block", [64, 100])
def test_query_blocks_merge_through_the_atomic(block, kind):
    N, K, D = 4099, 300, 70
    x, c = _gauss(1, N, D), _gauss(2, K, D)
    rows, x64, unit = _rows(kind, x)
    ct = torch.from_numpy(c).to(DEV)
    a, s = M.assign_clusters(rows, ct, block=block)
    _check_assign(a, s, ref.scores(x64, c, unit_rows=unit))
    a0, s0 = M.assign_clusters(rows, ct)
    assert _same_bits(a, a0) and _same_bits(s, s0)          # the same bits for any split of the centroids


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_equal_scores_go_to_the_lower_centroid(kind):
    K, D, N = 12, 70, 600
    rng = np.random.default_rng(7)
    c = ref.normalise(rng.standard_normal((K, D))).astype(np.float32)
    c[9] = c[3]                                             # a bit copy
    x = (c[np.arange(N) % K] + 0.03 * rng.standard_normal((N, D))).astype(np.float32)
    rows, x64, unit = _rows(kind, x)
    ra, _, _ = ref.assign(x64, c, unit_rows=unit)
    assert (ra != 9).all() and (ra == 3).sum() >= 2 * N // K
    a, s = M.assign_clusters(rows, torch.from_numpy(c).to(DEV))
    a, s = a.cpu().numpy(), s.cpu()
    assert (a != 9).all()
    a1, s1 = M.assign_clusters(rows, torch.from_numpy(np.delete(c, 9, axis=0)).to(DEV))
    on3 = ra == 3
    assert (a[on3] == 3).all() and (a1.cpu().numpy()[on3] == 3).all()
    assert (_bits(s)[on3] == _bits(s1)[on3]).all()


def _check_members(assign, K):
    N = assign.shape[0]
    offsets, order = M.cluster_members(torch.from_numpy(assign).to(DEV), K)
    offsets, order = offsets.cpu().numpy(), order.cpu().numpy()
    counts = np.bincount(assign, minlength=K)
    assert offsets.shape == (K + 1,) and (offsets == np.concatenate([[0], np.cumsum(counts)])).all()
    assert (np.sort(order) == np.arange(N)).all()
    for k in range(K):
        seg = order[offsets[k]: offsets[k + 1]]
        assert (assign[seg] == k).all() and (np.diff(seg) > 0).all()


def test_members():
    rng = np.random.default_rng(3)
    _check_members(rng.choice(np.array([0, 2, 5, 9]), 1000).astype(np.int64), 10)       # empty clusters
    _check_members(rng.integers(0, 70, 4099).astype(np.int64), 70)
    _check_members(np.zeros(257, np.int64), 1)
    _check_members(np.full(513, 4, np.int64), 5)                                         # all rows in the last cluster
    _check_members(np.zeros(1, np.int64), 1)
    _check_members(np.array([2], np.int64), 3)
    for bad in ([0, 3, 1], [0, -1, 1]):
        with pytest.raises(M.MI355Error, match="outside"):
            M.cluster_members(torch.tensor(bad, device=DEV), 3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [7, 70, 300])
def test_update_against_float64(D, kind):
    N, K = 900, 7
    x = _gauss(4, N, D).copy()
    x[N - 1] = -x[N - 2]                                    # cluster 6: two opposite rows, |sum| = 0 -> kept
    a = np.empty(N, np.int64)                               # cluster 0 empty, 1: 300 rows (two segments), 2: exactly 256
    a[:300], a[300:556], a[556:N - 2], a[N - 2:] = 1, 2, 3 + np.arange(N - 2 - 556) % 3, 6
    a[:N - 2] = a[:N - 2][np.random.default_rng(5).permutation(N - 2)]
    rows, x64, unit = _rows(kind, x)
    # the rows the update sums: a gallery's stored rows, or l2_normalize_rows of a raw tensor
    xn = x64 if unit else M.l2_normalize_rows(torch.from_numpy(x).to(DEV)).cpu().numpy().astype(np.float64)
    prev = _gauss(6, K, D)
    want, counts, kept = ref.update(xn, a, K, prev)
    assert kept.tolist() == [True, False, False, False, False, False, True]
    at, pt = torch.from_numpy(a).to(DEV), torch.from_numpy(prev).to(DEV)
    c, n, (offsets, order) = M.update_centroids(rows, at, K, pt)
    assert c.dtype == torch.float32 and c.shape == (K, D)
    cn = c.cpu().numpy()
    err = float(np.abs(cn[~kept].astype(np.float64) - want[~kept]).max())
    print(f"max |centroid - f64| {err:.3e} (bound {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23
    assert (cn[kept].view(np.int32) == prev[kept].view(np.int32)).all()
    assert n.dtype == torch.int64 and (n.cpu().numpy() == counts).all()
    assert (offsets.cpu().numpy() == np.concatenate([[0], np.cumsum(counts)])).all()
    assert (np.sort(order.cpu().numpy()) == np.arange(N)).all()
    c2, n2, _ = M.update_centroids(rows, at, K, pt)
    assert _same_bits(c, c2) and _same_bits(n, n2)
    with pytest.raises(M.MI355Error, match="outside"):
        M.update_centroids(rows, torch.full((N,), K, device=DEV), K, pt)


@functools.lru_cache(maxsize=None)
def _planted(cfg):
    x, lab, init = ref.planted(*cfg)
    return x, lab, init, ref.kmeans(x, init)


@pytest.mark.parametrize("gallery", [False, True])
@pytest.mark.parametrize("cfg", ref.PLANTED, ids=lambda c: "seed%d-%dx%d-k%d" % c[:4])
def test_loop_on_the_planted_inputs(cfg, gallery):
    x, lab, init, want = _planted(cfg)
    K = cfg[3]
    xt, it = torch.from_numpy(x).to(DEV), torch.from_numpy(init).to(DEV)
    if gallery:
        r = M.Gallery(x.shape[1], DEV).add(xt).kmeans(K, init=it)
    else:
        r = M.spherical_kmeans(xt, K, init=it)
    assert (r.assignments.cpu().numpy() == want["assignments"]).all()
    assert r.iterations == want["iterations"] and r.converged is True
    m = M.clustering_metrics(r.assignments, torch.from_numpy(lab).to(DEV))
    # NMI = 1.0 up to float64 rounding: 2I and H(a) + H(b) are sums of K logarithms taken in different orders, so the
    # quotient may differ from 1.0 in its last bits (each term <= ln K, a few ulp in all: far below 1e-12).  Purity and F1
    # are ratios of equal integers and are exactly 1.0.
    assert abs(m["nmi"] - 1.0) <= 1e-12 and m["purity"] == 1.0 and m["f1"] == 1.0
    assert (r.counts.cpu().numpy() == np.bincount(lab, minlength=K)).all()
    assert abs(r.objective - want["objectives"][-1]) <= 1e-5
    off, order = r.members
    assert (off.cpu().numpy() == np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=K))])).all()
    assert (lab[order.cpu().numpy()] == np.repeat(np.arange(K), np.bincount(lab, minlength=K))).all()


def _by_hand(rows, c, K, iters):
    last, objs, passes, updates = None, [], 0, 0
    while True:
        a, s = M.assign_clusters(rows, c)
        passes += 1
        objs.append(float(s.double().mean()))
        if (last is not None and torch.equal(a, last)) or updates == iters:
            return c, a, s, objs, passes
        c, _, _ = M.update_centroids(rows, a, K, c)
        updates += 1
        last = a


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_loop_is_its_two_primitives_and_the_objective_rises(kind):
    N, D, K = 3000, 72, 7
    rows, _, _ = _rows(kind, _gauss(9, N, D))
    init = torch.from_numpy(_gauss(10, K, D)).to(DEV)
    for iters in (3, 20):
        r = M.spherical_kmeans(rows, K, init=init, iters=iters)
        c, a, s, objs, passes = _by_hand(rows, init, K, iters)
        assert _same_bits(r.centroids, c) and _same_bits(r.assignments, a) and _same_bits(r.scores, s)
        assert r.iterations == passes and r.objective == objs[-1]
        assert (r.counts.cpu().numpy() == np.bincount(a.cpu().numpy(), minlength=K)).all()
    drops = [objs[i] - objs[i + 1] for i in range(len(objs) - 1)]
    print("objective per pass", objs)
    assert len(objs) >= 3 and max(drops) <= 1e-6


def test_seeded_start_is_deterministic():
    N, D, K = 3000, 72, 7
    x = torch.from_numpy(_gauss(9, N, D)).to(DEV)
    r1, r2 = M.spherical_kmeans(x, K, seed=5, iters=4), M.spherical_kmeans(x, K, seed=5, iters=4)
    assert _same_bits(r1.centroids, r2.centroids) and _same_bits(r1.assignments, r2.assignments)
    assert _same_bits(r1.scores, r2.scores) and r1.objective == r2.objective
    r0 = M.spherical_kmeans(x, K, seed=5, iters=0)           # the start itself: K distinct rows
    from imageretrievalresearch_amd.cluster import seeded_rows
    assert _same_bits(r0.centroids, x[torch.from_numpy(seeded_rows(N, K, 5)).to(DEV)])
    assert r0.iterations == 1 and not r0.converged
    with pytest.raises(M.MI355Error, match="finite"):
        M.spherical_kmeans(torch.full((8, 4), float("nan"), device=DEV), 2)


@pytest.mark.parametrize("N,Ka,Kb", [(5000, 7, 5), (5000, 100, 100), (1, 1, 1), (4099, 8192, 1), (3000, 91, 91)])
def test_contingency_and_metrics(N, Ka, Kb):
    rng = np.random.default_rng(N + Ka)
    av = np.sort(rng.choice(np.arange(-5 * Ka, 5 * Ka), Ka, replace=False)).astype(np.int64)     # gaps and negatives
    bv = np.sort(rng.choice(np.arange(-3 * Kb, 9 * Kb), Kb, replace=False)).astype(np.int64)
    a, b = av[rng.integers(0, Ka, N)], bv[rng.integers(0, Kb, N)]
    want, wa, wb = ref.contingency(a, b)
    at, bt = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    t, ta, tb = M.contingency(at, bt)
    assert t.dtype == torch.int64 and (t.cpu().numpy() == want).all()
    assert (ta.cpu().numpy() == wa).all() and (tb.cpu().numpy() == wb).all()
    got, m = M.clustering_metrics(at, bt), ref.metrics(a, b)
    for k in ("nmi", "purity", "f1", "precision", "recall"):
        assert abs(got[k] - m[k]) <= 1e-12, k
    assert got["n_clusters"] == m["n_clusters"] and got["n_classes"] == m["n_classes"]


@pytest.mark.parametrize("Ka,Kb", [(128, 64), (8192, 1), (8193, 1), (2731, 3)])
def test_contingency_at_the_lds_table_limit(Ka, Kb):
    # 8192 cells is the last table kept as LDS sub-histograms, 8193 the first counted with global atomics.  Every id occurs,
    # so the dense table has exactly Ka x Kb cells.
    N = 20000
    rng = np.random.default_rng(Ka * Kb)
    a = rng.permutation(np.concatenate([np.arange(Ka), rng.integers(0, Ka, N - Ka)])).astype(np.int64)
    b = rng.permutation(np.concatenate([np.arange(Kb), rng.integers(0, Kb, N - Kb)])).astype(np.int64)
    want = np.zeros((Ka, Kb), np.int64)
    np.add.at(want, (a, b), 1)
    t, ta, tb = M.contingency(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert tuple(t.shape) == (Ka, Kb) and (t.cpu().numpy() == want).all() and int(t.sum()) == N
    assert (ta.cpu().numpy() == np.arange(Ka)).all() and (tb.cpu().numpy() == np.arange(Kb)).all()


def test_contingency_reports_ids_out_of_range():
    L, ws = M.lib(), torch.empty(1024, dtype=torch.uint8, device=DEV)
    a, b = torch.tensor([0, 1, 2], device=DEV), torch.tensor([0, 5, 1], device=DEV)
    table = torch.empty(6, dtype=torch.int64, device=DEV)
    st = L.mi355_contingency(a.data_ptr(), b.data_ptr(), 3, 3, 2, table.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert st != 0 and b"outside" in L.mi355_last_error()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_gallery_clustering_metrics_is_the_composition(dtype):
    x, lab, _, _ = _planted(ref.PLANTED[0])
    labels = torch.from_numpy(lab * 11 - 40).to(DEV)
    g = M.Gallery(x.shape[1], DEV, dtype=dtype).add(torch.from_numpy(x).to(DEV), labels)
    got = g.clustering_metrics(seed=2)
    r = g.kmeans(9, seed=2)
    assert got == M.clustering_metrics(r.assignments, labels) and got["n_classes"] == 9
    assert g.clustering_metrics(4, iters=2) == M.clustering_metrics(g.kmeans(4, iters=2).assignments, labels)
    with pytest.raises(M.MI355Error, match="labels"):
        M.Gallery(4, DEV).add(torch.ones(3, 4, device=DEV)).clustering_metrics()
