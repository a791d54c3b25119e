"""k-reciprocal re-ranking without a GPU: argument errors of the four mi355_kr_* entries (rejected before any HIP call) and of
the Python API, and the float64 reference (tests/rerank_ref.py) against hand-worked examples and its own invariants."""
import math

import numpy as np
import pytest
import torch

import rerank_ref as rr
from imageretrievalresearch_amd import MI355Error, _lib, k_reciprocal_rerank
from imageretrievalresearch_amd import rank as R
from imageretrievalresearch_amd import rerank as K

F32, F16 = _lib.DTYPE_F32, _lib.DTYPE_F16


def _err():
    return _lib.lib().mi355_last_error()


def _sets(lists=1, lvals=None, tau=None, R_=10, k1=5, graph=1, G=10, offsets=1, cols=None, cap=0):
    return _lib.lib().mi355_kr_sets(lists, lvals, tau, R_, k1, graph, G, offsets, cols, cap, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(lists=None), b"null"), (dict(graph=None), b"null"), (dict(offsets=None), b"null"), (dict(k1=0), b"k1=0"),
    (dict(k1=33), b"k1=33"), (dict(R_=-1), b"bad shape"), (dict(G=0), b"bad shape"), (dict(lvals=1), b"both"), (dict(tau=1), b"both"),
    (dict(R_=9), b"whole graph"), (dict(cols=1, cap=-1), b"cols_capacity"),
])
def test_kr_sets_rejects_bad_arguments(kw, msg):
    assert _sets(**kw) != 0
    assert msg in _err(), (kw, _err())


def _weights(rows=1, rdt=F32, rld=8, R_=4, gal=1, gdt=F32, G=10, gld=8, dim=8, offsets=1, cols=1, nnz=5, vals=1):
    return _lib.lib().mi355_kr_weights(rows, rdt, rld, R_, gal, gdt, G, gld, dim, offsets, cols, nnz, vals, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(rows=None), b"null"), (dict(gal=None), b"null"), (dict(offsets=None), b"null"), (dict(cols=None), b"needs cols"),
    (dict(vals=None), b"needs cols"), (dict(nnz=-1), b"nnz"), (dict(rdt=5), b"dtype"), (dict(gdt=-1), b"dtype"), (dict(dim=0), b"dim"),
    (dict(dim=8193, rld=8193, gld=8193), b"dim"), (dict(rld=7), b"leading dims"), (dict(gld=4), b"leading dims"),
    (dict(R_=-2), b"bad shape"), (dict(G=0), b"bad shape"),
])
def test_kr_weights_rejects_bad_arguments(kw, msg):
    assert _weights(**kw) != 0
    assert msg in _err(), (kw, _err())


def _local(lists=1, R_=4, k1=5, k2=3, oo=1, oc=1, ov=1, onnz=3, go=1, gc=1, gv=1, gnnz=3, G=10, out_o=1, out_c=None, out_v=None, cap=0):
    return _lib.lib().mi355_kr_local_qe(lists, R_, k1, k2, oo, oc, ov, onnz, go, gc, gv, gnnz, G, out_o, out_c, out_v, cap, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(lists=None), b"null"), (dict(oo=None), b"null"), (dict(go=None), b"null"), (dict(out_o=None), b"null"),
    (dict(k1=40), b"k1=40"), (dict(k2=0), b"k2=0"), (dict(k2=7), b"k2=7"), (dict(oc=None), b"own_nnz"), (dict(gv=None), b"gallery_nnz"),
    (dict(out_c=1), b"both"), (dict(out_c=1, out_v=1, cap=-3), b"out_capacity"), (dict(R_=-1), b"bad shape"),
])
def test_kr_local_qe_rejects_bad_arguments(kw, msg):
    assert _local(**kw) != 0
    assert msg in _err(), (kw, _err())


def _score(qo=1, qc=1, qv=1, qnnz=3, Q=4, go=1, gc=1, gv=1, gnnz=3, G=10, sv=1, si=1, K_=5, lam=0.3, out=1):
    return _lib.lib().mi355_kr_score(qo, qc, qv, qnnz, Q, go, gc, gv, gnnz, G, sv, si, K_, lam, out, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(qo=None), b"null"), (dict(go=None), b"null"), (dict(sv=None), b"null"), (dict(si=None), b"null"), (dict(out=None), b"null"),
    (dict(K_=0), b"K=0"), (dict(K_=1025), b"K=1025"), (dict(lam=-0.5), b"lam"), (dict(lam=1.5), b"lam"), (dict(lam=math.nan), b"lam"),
    (dict(qc=None), b"query_nnz"), (dict(gc=None), b"gallery_nnz"), (dict(Q=-1), b"bad shape"), (dict(G=0), b"bad shape"),
])
def test_kr_score_rejects_bad_arguments(kw, msg):
    assert _score(**kw) != 0
    assert msg in _err(), (kw, _err())


def test_zero_rows_do_nothing():
    assert _sets(R_=0, lvals=1, tau=1) == 0 and _weights(R_=0) == 0 and _weights(nnz=0, cols=None, vals=None) == 0
    assert _local(R_=0) == 0 and _score(Q=0) == 0


def test_python_parameters():
    assert K.rerank_params(300, 5) == (5, 20, 6, 0.3, 100)
    assert K.rerank_params(50, 5) == (5, 20, 6, 0.3, 50)               # shortlist default: min(G, max(k, 100))
    assert K.rerank_params(3000, 150, shortlist=None)[4] == 150
    assert K.rerank_params(40, 40, k1=32, k2=33, lam=1, shortlist=40) == (40, 32, 33, 1.0, 40)
    for kw in (dict(k1=0), dict(k1=33), dict(k1=True), dict(k1=2.0), dict(k2=0), dict(k2=22), dict(lam=-1e-9), dict(lam=1.0001),
               dict(lam=float("nan")), dict(lam=float("inf")), dict(lam="x"), dict(shortlist=4), dict(shortlist=301),
               dict(shortlist=10.0)):
        with pytest.raises(MI355Error):
            K.rerank_params(300, 5, **kw)
    for G, k, kw in ((20, 5, {}), (21, 5, dict(k1=21)), (3000, 5, dict(shortlist=1025)), (3000, 1025, {}), (300, 0, {}), (300, True, {})):
        with pytest.raises(MI355Error):
            K.rerank_params(G, k, **kw)


def test_python_api_rejects_cpu_tensors():
    q, g = torch.randn(4, 8), torch.randn(40, 8)
    with pytest.raises(MI355Error, match="GPU"):
        k_reciprocal_rerank(q, g, 2)
    gal = R.Gallery(8, "cpu")
    with pytest.raises(MI355Error):
        gal.rerank(q, 2)
    with pytest.raises(MI355Error):
        gal.knn_graph(20)                                       # k1 >= rows
    with pytest.raises(MI355Error):
        gal.rerank_index(0, 1)
    with pytest.raises(MI355Error, match="GPU"):
        K._kr_sets(torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 3, dtype=torch.int64))


# six rows, k1 = 2 (h = 1): 0-1 and 2-3 are mutual first neighbours, 4 -> 3, 5 -> 4
GRAPH = np.array([[1, 2], [0, 2], [3, 1], [2, 4], [3, 5], [4, 3]])


def test_reference_sets_by_hand():
    assert rr.recip_h(GRAPH, 0, 1) == {0, 1} and rr.recip_h(GRAPH, 2, 1) == {2, 3} and rr.recip_h(GRAPH, 4, 1) == {4}
    assert rr.base_set(0, GRAPH[0], GRAPH) == {0, 1}              # 0 is in nn(1), not in nn(2)
    assert rr.base_set(2, GRAPH[2], GRAPH) == {1, 2, 3} and rr.base_set(3, GRAPH[3], GRAPH) == {2, 3, 4}
    # R(2) = {1, 2, 3}: R_h(1) = {0, 1} shares 1 of 2 (3 > 4 fails), R_h(2) = R_h(3) = {2, 3} are inside already
    assert rr.sets(GRAPH, GRAPH) == [[0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5], [4, 5]]
    # a larger neighbourhood: R_h(c) = {c, a, b, x} with three of four inside R brings x in (9 > 8)
    g3 = np.array([[1, 2, 3, 9, 9, 9], [0, 2, 3, 9, 9, 9], [0, 1, 4, 9, 9, 9], [0, 1, 9, 9, 9, 9], [2, 9, 9, 9, 9, 9]]
                  + [[9, 9, 9, 9, 9, 9]] * 5)
    assert rr.recip_h(g3, 2, 3) == {0, 1, 2, 4}
    assert rr.expanded_set({0, 1, 2}, g3, 3) == {0, 1, 2, 3, 4}    # 3 through R_h(0) = {0, 1, 2, 3}, 4 through R_h(2)
    # query rows: fp32 comparison with tau, equality included; an empty R(q) stays empty
    tau = np.array([0.5, 0.5, 0.25, 0.5, 0.5, 0.5], np.float32)
    lists, vals = np.array([[2, 0], [4, 5]]), np.array([[0.25, 0.1], [0.4, 0.3]], np.float32)
    assert rr.sets(lists, GRAPH, vals, tau) == [[2], []]


def test_reference_invariants():
    rng = np.random.default_rng(0)
    G, D, k1, k2 = 60, 12, 6, 3
    x = rng.standard_normal((G + 5, D))
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    gn, qn = xn[:G], xn[G:]
    gnv, gnn = rr.knn(gn, gn, k1, np.arange(G))
    assert (gnn != np.arange(G)[:, None]).all() and (np.diff(gnv.astype(np.float64), axis=1) <= 0).all()
    S = rr.sets(gnn, gnn)
    h = (k1 + 1) // 2
    for g, s in enumerate(S):
        assert g in s and s == sorted(set(s)) and len(s) <= (k1 + 1) * (h + 1)
        assert rr.base_set(g, gnn[g], gnn) <= set(s)
    assert any(len(s) > len(rr.base_set(g, gnn[g], gnn)) for g, s in enumerate(S))      # some set does expand
    # reciprocity of the unexpanded sets is symmetric
    for g in range(G):
        for j in rr.base_set(g, gnn[g], gnn):
            assert g in rr.base_set(j, gnn[j], gnn)
    V, V2 = rr.gallery_index(gn, gnn, k2)
    for v, v2 in zip(V, V2):
        assert abs(sum(v.values()) - 1) < 1e-12 and abs(sum(v2.values()) - 1) < 1e-12 and min(v.values()) > 0
    assert rr.local_qe(V, V, gnn, 1) == V                        # k2 = 1: V itself
    sv, si = rr.knn(qn, gn, 10)
    tau = gnv[:, -1]
    far = rr.sets(si[:, :k1], gnn, np.full((5, k1), -1, np.float32), tau)
    assert all(s == [] for s in far)                             # below every tau: empty sets, empty V, dJ = 1
    s_far = rr.scores(rr.local_qe(rr.weights(qn, gn, far), [{} for _ in V], si[:, :k1], 1), V2, sv, si, 0.3)
    np.testing.assert_allclose(s_far, 1 - (0.7 + 0.3 * (1 - sv.astype(np.float64))), atol=1e-15)
    for lam in (0.0, 0.3, 1.0):
        s = rr.pipeline(qn, gn, gnv, gnn, sv[:, :k1], si[:, :k1], sv, si, k2, lam)
        assert s.shape == (5, 10) and (s <= 1 + 1e-12).all()
        if lam == 1.0:                                           # the plain search: same values, same order
            np.testing.assert_allclose(s, sv.astype(np.float64), atol=1e-15)
            assert np.array_equal(rr.rank_shortlist(s, si, 4)[1], si[:, :4])
    # a gallery row as its own query with full overlap: m = 1, dJ = 0, s* = 1 - lam (1 - s)
    s_self = rr.scores([V2[7]], V2, np.array([[0.5]]), np.array([[7]]), 0.3)
    np.testing.assert_allclose(s_self, [[1 - 0.3 * 0.5]], atol=1e-12)
    # pads stay pads, ties keep the earlier position
    sp = rr.scores([V2[7]], V2, np.array([[0.5, -np.inf]]), np.array([[7, -1]]), 0.3)
    assert sp[0, 1] == -np.inf
    v, i, pos = rr.rank_shortlist(np.array([[0.2, 0.9, 0.9, -np.inf]]), np.array([[5, 6, 7, -1]]), 4)
    assert i.tolist() == [[6, 7, 5, -1]] and pos.tolist() == [[1, 2, 0, 3]]
    assert rr.gaps(np.array([[0.9, 0.5, 0.49, 0.1]]), 2)[0] == pytest.approx(0.01)
