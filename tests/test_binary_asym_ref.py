"""The asymmetric binary search's contract on the CPU: the identities of the weighted distance, the order, the special queries,
and the recall condition the feature is for - stated on the NumPy model (binary_asym_ref.py), which the GPU reproduces bit
for bit (tests/test_binary_asym_gpu.py)."""
import numpy as np
import pytest

import binary_asym_ref as A
import binary_ref as R


def _case(seed, G=300, Q=9, D=130):
    r = np.random.default_rng(seed)
    n, qn = R.normalize(r.standard_normal((G, D))), R.normalize(r.standard_normal((Q, D)))
    c = (0.5 * r.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    return n, qn, c


@pytest.mark.parametrize("seed", [0, 1])
def test_distance_identities(seed):
    n, qn, c = _case(seed)
    g = R.encode(n, c)
    m, s, u, l1, nan = A.model(qn, g, c)
    assert not nan.any() and (np.abs(u).max(axis=1) == 127).all()         # the largest |r| of a row gets the full code
    assert (m == A.weighted_distances_by_definition(u, g)).all()
    sgn = 2 * A.bits(g, n.shape[1]).astype(np.int64) - 1                  # s_j = 2 bit_j - 1
    assert (l1[:, None] - 2 * m.astype(np.int64) == u.astype(np.int64) @ sgn.T).all()
    assert (m >= 0).all() and (m <= l1[:, None]).all()
    # a row that agrees with the query's signs everywhere is at 0, its complement at L1
    own = R.encode(qn, c)
    assert (np.diag(A.weighted_distances(u, own)) == 0).all()
    assert (np.diag(A.weighted_distances(u, ~own)) == l1).all()
    # with every weight 1 it is the symmetric distance, but for the elements whose code is 0
    h = R.distances(own, g).astype(np.int64)
    w1 = np.sign(u).astype(np.int8)
    gap = h - A.weighted_distances(w1, g)
    assert (gap >= 0).all() and (gap <= (w1 == 0).sum(axis=1)[:, None]).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_order_by_score_is_order_by_distance_then_row(seed):
    n, qn, c = _case(seed, G=2000)
    n[500:520] = n[3]                                                     # ties
    g = R.encode(n, c)
    m, s, u, l1, _ = A.model(qn, g, c)
    for k in (1, 10, 2000):
        _, idx = R.select(s, k)
        want = np.lexsort((np.broadcast_to(np.arange(m.shape[1]), m.shape), m), axis=1)[:, :k]
        assert (idx == want).all()
    # distinct distances give distinct scores, also at the largest L1 = 127 * 65536
    L = np.array([127 * 65536], np.int64)
    mm = np.arange(0, 127 * 65536 + 1, 4099, dtype=np.int64)[None, :]
    near = np.concatenate([mm, mm + 1], axis=1)
    near = np.sort(near[near <= L[0]])[None, :]
    sc = A.scores(near, L)
    assert (np.diff(sc[0]) < 0).all()
    assert sc[0, 0] == np.float32(1.0) and A.scores(L[None, :], L)[0, 0] == np.float32(-1.0)


def test_special_queries():
    n, qn, c = _case(5)
    g = R.encode(n, c)
    q = qn.copy()
    q[1, 7] = np.nan                                                      # a NaN query
    q[2] = c                                                              # r == 0: L1 == 0
    q[3] = c + np.float32(1e-35)                                          # amax < 1e-30
    q[4, 0] = np.inf                                                      # a non-finite amax
    m, s, u, l1, nan = A.model(q, g, c)
    assert nan.tolist() == [False, True, False, False, True] + [False] * 4
    assert (m[[1, 4]] == -1).all() and np.isnan(s[[1, 4]]).all() and (u[[1, 2, 3, 4]] == 0).all()
    assert (l1[[1, 2, 3, 4]] == 0).all() and (m[[2, 3]] == 0).all()
    assert (s[[2, 3]] == 0).all() and not np.signbit(s[[2, 3]]).any()     # +0.0 against every row
    _, idx = R.select(s[[1, 2]], 5)
    assert (idx == np.arange(5)[None, :]).all()                           # all tied: the rows in order
    zero = np.zeros((1, n.shape[1]), np.float32)                          # a zero query with a zero centre
    m0, s0, u0, l0, nan0 = A.model(zero, g, None)
    assert not nan0[0] and l0[0] == 0 and (s0 == 0).all() and (m0 == 0).all()


@pytest.mark.parametrize("pooled", [False, True], ids=["raw", "pooled"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_asymmetric_shortlist_recalls_more(seed, pooled):
    """Refined recall@10 on the planted mixture, mean centre: at a shortlist of 30 the asymmetric search is at least 0.05 above
    the symmetric one, and both reach 0.95 at a shortlist of 100."""
    n, qn = A.mixture_rows(seed, pooled)
    c = R.mean_center(n)
    g, qc = R.encode(n, c), R.encode(qn, c)
    sym = R.scores(R.distances(qc, g), n.shape[1])
    _, asym, u, l1, _ = A.model(qn, g, c)
    got = {}
    for short in (30, 100):
        got[short] = (R.refined_recall(n, qn, g, qc, 10, short), A.refined_recall(n, qn, asym, 10, short))
        assert A.refined_recall(n, qn, sym, 10, short) == got[short][0]   # the keyed routine is binary_ref's on the same key
    distinct = (np.mean([len(np.unique(r)) for r in sym]), np.mean([len(np.unique(r)) for r in asym]))
    print(f"seed {seed} {'pooled' if pooled else 'raw'}: refined recall@10 symmetric / asymmetric at 30: {got[30][0]:.4f} / "
          f"{got[30][1]:.4f}, at 100: {got[100][0]:.4f} / {got[100][1]:.4f}; distinct scores per query {distinct[0]:.0f} / "
          f"{distinct[1]:.0f}")
    assert got[30][1] >= got[30][0] + 0.05
    assert got[100][0] >= 0.95 and got[100][1] >= 0.95
