"""retrieval_accuracy on the GPU: the metrics kernel against a numpy float64 computation of the four definitions on the same
ranking, the whole pipeline against a float64 ranking on well-separated clusters, lone labels, cross-source evaluation,
R from 1 to 1024, and the error for R > 1024."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import MI355Error

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (1, 2, 4, 8)


def _np_metrics(idx, ql, gl, R, ks):
    """Float64 reference of precision@1, recall@K, R-precision and MAP@R (Musgrave et al. 2020) for ranked rows idx."""
    idx, ql, gl, R = (t.cpu().numpy() for t in (idx, ql, gl, R))
    G = gl.shape[0]
    valid = R > 0
    rel = np.where((idx >= 0) & (idx < G), gl[np.clip(idx, 0, G - 1)] == ql[:, None], False)
    p1 = rel[:, 0].astype(np.float64)
    rec = {K: rel[:, :K].any(1).astype(np.float64) for K in ks}
    rp = np.zeros(len(R))
    mapr = np.zeros(len(R))
    for q in np.nonzero(valid)[0]:
        r = int(R[q])
        rr = rel[q, :r].astype(np.float64)
        rp[q] = rr.sum() / r
        mapr[q] = (rr * np.cumsum(rr) / np.arange(1, r + 1)).sum() / r
    m = lambda x: x[valid].mean()
    return {"precision_at_1": m(p1), "recall_at_k": {K: m(rec[K]) for K in ks}, "r_precision": m(rp), "map_at_r": m(mapr),
            "per_query": (rp, mapr), "num_lone": int((~valid).sum())}


def _compare(got, want, tol):
    assert abs(got["precision_at_1"].item() - want["precision_at_1"]) <= tol
    for K in want["recall_at_k"]:
        assert abs(got["recall_at_k"][K].item() - want["recall_at_k"][K]) <= tol, K
    assert abs(got["r_precision"].item() - want["r_precision"]) <= tol
    assert abs(got["map_at_r"].item() - want["map_at_r"]) <= tol
    assert int(got["num_lone"]) == want["num_lone"]


def _data(n, D, classes, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(classes, D, generator=g)               # first: the same seed gives the same centres for any n
    lab = torch.randint(0, classes, (n,), generator=g)
    x = centers[lab] + spread * torch.randn(n, D, generator=g)
    return x.to(DEV), lab.to(DEV)


@pytest.mark.parametrize("classes", [5, 50, 400])
def test_kernel_metrics_equal_float64_on_the_library_ranking(classes):
    x, lab = _data(3000, 128, classes, classes, spread=3.0)      # overlapping classes: every metric strictly inside (0, 1)
    lab[:7] = 10_000 + torch.arange(7, device=DEV)               # lone labels
    got = M.retrieval_accuracy(x, lab, ks=KS)
    want = _np_metrics(got["indices"], lab, lab, got["R"], KS)
    _compare(got, want, 1e-6)
    rp, mapr = want["per_query"]
    per = got["per_query"].cpu().numpy()
    v = got["R"].cpu().numpy() > 0
    assert np.abs(per[v, 1] - rp[v]).max() <= 1e-12 and np.abs(per[v, 2] - mapr[v]).max() <= 1e-12
    assert got["num_queries"] == 3000 and int(got["num_lone"]) >= 7           # (+ classes drawn once at 400 classes)
    assert 0 < want["map_at_r"] < 1 and 0 < want["precision_at_1"] < 1


def _f64_pipeline(q, ql, g, gl, ks, same_source):
    qn = q.double() / q.double().norm(dim=1, keepdim=True)
    gn = g.double() / g.double().norm(dim=1, keepdim=True)
    s = qn @ gn.t()
    if same_source:
        s.fill_diagonal_(-float("inf"))
    counts = (gl[None, :] == ql[:, None]).sum(1) - (1 if same_source else 0)
    k = min(max(max(ks), int(counts.max())), g.shape[0])
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    if same_source:
        order[torch.gather(s, 1, order) == -float("inf")] = -1
    return _np_metrics(order, ql, gl, counts, ks)


def test_end_to_end_equals_float64_on_separated_clusters():
    x, lab = _data(4000, 256, 40, 7, spread=0.05)
    got = M.retrieval_accuracy(x, lab, ks=KS)
    want = _f64_pipeline(x, lab, x, lab, KS, True)
    _compare(got, want, 0.0)
    assert want["map_at_r"] == 1.0


def test_cross_source_queries_against_a_gallery():
    g, gl = _data(5000, 96, 30, 11, spread=2.5)
    q, ql = _data(700, 96, 30, 11, spread=2.5)                  # same class centres (same seed), other samples
    ql[:5] = 999                                                 # not in the gallery: lone
    got = M.retrieval_accuracy(q, ql, g, gl, ks=(1, 5, 10))
    want = _np_metrics(got["indices"], ql, gl, got["R"], (1, 5, 10))
    _compare(got, want, 1e-6)
    assert int(got["num_lone"]) == 5
    ref = _f64_pipeline(q, ql, g, gl, (1, 5, 10), False)
    assert abs(got["map_at_r"].item() - ref["map_at_r"]) <= 1e-3   # rankings may differ at fp32 near-ties only
    with pytest.raises(MI355Error, match="gallery_labels"):
        M.retrieval_accuracy(q, ql, g)


@pytest.mark.parametrize("R", [1, 2, 63, 64, 65, 500, 1024])
def test_class_sizes_from_1_to_1024(R):
    n = R + 1                                                    # one class of R + 1 rows: R relevant rows per query
    x, _ = _data(n + 300, 64, 1, R, spread=1.0)
    lab = torch.cat([torch.zeros(n, dtype=torch.int64), 1 + torch.arange(300) % 150]).to(DEV)
    got = M.retrieval_accuracy(x, lab, ks=KS)
    want = _np_metrics(got["indices"], lab, lab, got["R"], KS)
    _compare(got, want, 1e-6)
    assert int(got["R"].max()) == R and got["indices"].shape[1] == max(R, 8)


def test_more_than_1024_relevant_rows_raise_naming_the_class():
    x, _ = _data(1100, 32, 1, 3)
    lab = torch.full((1100,), 42, dtype=torch.int64, device=DEV)
    lab[:50] = 7
    with pytest.raises(MI355Error, match="class 42 has 1049"):
        M.retrieval_accuracy(x, lab)
    with pytest.raises(MI355Error, match="ks must be"):
        M.retrieval_accuracy(x, lab, ks=(0, 1))
