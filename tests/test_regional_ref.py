"""The float64 model of the regional MaxSim score (tests/regional_ref.py) against brute-force loops on tiny inputs, and the
retrieval value of the planted-part fixture in the model itself.  No GPU."""
import numpy as np
import pytest

import regional_ref as RR


def _brute(qh, gh, w):
    Q, Rq, dim = qh.shape
    G, R, _ = gh.shape
    sc, am = np.zeros((Q, G)), np.zeros((Q, G, Rq), np.int32)
    for q in range(Q):
        for g in range(G):
            total = 0.0
            for i in range(Rq):
                best, at = None, -1
                for j in range(R):
                    s = 0.0
                    for d in range(dim):
                        s += float(qh[q, i, d]) * float(gh[g, j, d])
                    if best is None or s > best:
                        best, at = s, j
                total += w[q, i] * best
                am[q, g, i] = at
            sc[q, g] = total
    return sc, am


@pytest.mark.parametrize("Rq, R, dim", [(1, 1, 3), (3, 5, 7), (4, 2, 9)])
def test_scores_and_matches_equal_brute_force(Rq, R, dim):
    qh = RR.codes(RR.random_regions(1, 3, Rq, dim))
    gh = RR.codes(RR.random_regions(2, 6, R, dim))
    for w in (None, np.random.default_rng(3).standard_normal((3, Rq)).astype(np.float32)):
        sc, am, gap = RR.scores(qh, gh, None, w)
        wd = RR.default_weights(3, Rq) if w is None else w.astype(np.float64)
        bs, ba = _brute(qh, gh, wd)
        assert np.abs(sc - bs).max() < 1e-12 and (am == ba).all()
        assert (gap >= 0).all() and (np.isinf(gap).all() if R == 1 else np.isfinite(gap).all())


def test_codes_are_fp16_unit_vectors_and_zero_rows_stay_zero():
    x = RR.random_regions(4, 2, 3, 20)
    x[1, 2] = 0
    c = RR.codes(x)
    assert c.dtype == np.float16 and (c[1, 2] == 0).all()
    n = np.sqrt((c.astype(np.float64) ** 2).sum(-1))
    assert np.abs(np.delete(n.reshape(-1), 5) - 1).max() < 2e-3
    assert RR.default_weights(2, 3)[0, 0] == np.float64(np.float32(1) / np.float32(3))


def test_ties_go_to_the_lower_region_and_pads_score_minus_inf():
    qh = RR.codes(RR.random_regions(5, 2, 3, 8))
    gh = RR.codes(RR.random_regions(6, 4, 4, 8))
    gh[:, 3] = gh[:, 1]                                          # identical bits: region 1 must win over region 3
    idx = np.array([[-1, 2, 2, 0, 4], [3, -1, 1, 1, -1]])        # pads front / middle / end, a row twice, 4 = outside
    sc, am, gap = RR.scores(qh, gh, idx)
    full, fa, _ = RR.scores(qh, gh)
    assert (am != 3).all() and (fa != 3).all()
    pad = (idx < 0) | (idx >= 4)
    assert np.isneginf(sc[pad]).all() and (am[pad] == -1).all() and np.isinf(gap[pad]).all()
    assert sc[0, 1] == sc[0, 2] == full[0, 2] and sc[1, 2] == full[1, 1] and (am[0, 3] == fa[0, 0]).all()


def test_topk_search_and_rerank_order():
    s = np.array([[0.5, 0.9, 0.9, -np.inf, 0.1]])
    v, i, pos = RR.topk(s, 5, idx_offset=10)
    assert i.tolist() == [[11, 12, 10, 14, -1]] and np.isneginf(v[0, 4]) and pos.tolist() == [[1, 2, 0, 4, 3]]
    qh = RR.codes(RR.random_regions(7, 3, 2, 6))
    gh = RR.codes(RR.random_regions(8, 9, 3, 6))
    v, i, slab = RR.search(qh, gh, 9, exclude=np.array([104, 100, 999]), idx_offset=100)
    assert i[0, -1] == -1 and i[1, -1] == -1 and i[2, -1] >= 100 and 104 not in i[0] and 100 not in i[1]
    assert (np.diff(v, axis=1) <= 0).all()
    sl = np.array([[4, 4, 1, -1], [0, 8, -1, 2], [7, 6, 5, 4]])
    rv, ri, rm, rs = RR.rerank(qh, gh, sl, 4, idx_offset=50)
    assert ri[0, -1] == -1 and ri[1, -1] == -1 and (ri[2] >= 50).all() and np.isneginf(rv[0, -1])
    assert ri[0, 0] == 54 or ri[0, 0] == 51
    assert list(ri[0]).count(54) == 2 and rm.shape == (3, 4, 2) and (rm[0, -1] == -1).all()


def test_pooled_rows_are_the_normalised_sums():
    gh = RR.codes(RR.random_regions(9, 4, 5, 12))
    p = RR.pooled(gh)
    x = gh.astype(np.float64).sum(1)
    assert np.abs(p - x / np.linalg.norm(x, axis=1, keepdims=True)).max() < 1e-15
    assert RR.tol(128, 14) == pytest.approx(8.46e-6, rel=1e-2)
    assert RR.tol(128, 14, np.full((2, 14), 0.5)) == pytest.approx(7 * 8.46e-6, rel=1e-2)


def test_all_negative_fixture_is_all_negative():
    q, g = RR.all_negative(11, 4, 9, 3, 40)
    s = RR.pair_tables(RR.codes(q), RR.codes(g))
    assert s.max() < -0.5
    assert RR.scores(RR.codes(q), RR.codes(g))[0].max() < -0.5


@pytest.mark.parametrize("dim", [128, 64])
def test_planted_part_fixture_regional_matching_finds_what_the_pooled_row_loses(dim):
    """The retrieval value the feature is for, in the model: precision@1 of the exhaustive regional search and of the re-ranked
    global top-100 is >= 0.95, that of the pooled (R-MAC) rows <= 0.30."""
    g, gl, q, ql = RR.planted_parts(dim=dim)
    gh, qh = RR.codes(g), RR.codes(q)
    _, si, _ = RR.search(qh, gh, 1)
    rows, qrows = RR.pooled(gh), RR.pooled(qh)
    short = RR.global_shortlist(qrows, rows, 100)
    _, ri, _, _ = RR.rerank(qh, gh, short, 1)
    p_search, p_rerank = RR.precision_at_1(si[:, 0], ql, gl), RR.precision_at_1(ri[:, 0], ql, gl)
    p_pooled = RR.precision_at_1(short[:, 0], ql, gl)
    print(f"dim {dim}: precision@1 regional search {p_search:.2f}, rerank of the global top-100 {p_rerank:.2f}, pooled rows {p_pooled:.2f}")
    assert p_search >= 0.95 and p_rerank >= 0.95 and p_pooled <= 0.30
