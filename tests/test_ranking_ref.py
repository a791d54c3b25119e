"""The CPU reference of the ranking metrics (tests/ranking_ref.py) against the definitions restated pair by pair, on
hand-written cases: ties at both index orders, a lone query, an excluded best positive, NaN and signed zeros."""
import numpy as np

import ranking_ref as RR


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), (a, b)


def test_score_keys_order():
    s = np.array([-np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-30, 0.5, 1.0, np.inf, np.nan], dtype=np.float32)
    k = RR.score_keys(s).astype(np.int64)
    assert k[3] == k[4]                                  # -0 == +0
    assert (np.diff(np.delete(k, 3)) > 0).all()          # otherwise strictly ascending, NaN the largest
    assert k[-1] == 0xFFFFFFFF and k[0] > 0


def test_tie_between_a_positive_and_a_negative_at_both_index_orders():
    # query 0 (label 1): positive row 2 ties with negative row 1 (lower row: the negative ranks first -> rank 3)
    # query 1 (label 1): positive row 0 ties with negative row 3 (lower row: the positive ranks first -> rank 1)
    S = np.array([[0.9, 0.5, 0.5, 0.1],
                  [0.5, 0.2, 0.1, 0.5]], dtype=np.float32)
    gl = np.array([0, 0, 1, 0])
    off, idx, ranks, ap, first = RR.rank_positives(S[:1], [1], gl)
    assert idx.tolist() == [2] and ranks.tolist() == [3] and ap[0] == 1.0 / 3.0 and first.tolist() == [3]
    gl2 = np.array([1, 0, 0, 0])
    off, idx, ranks, ap, first = RR.rank_positives(S[1:], [1], gl2)
    assert idx.tolist() == [0] and ranks.tolist() == [1] and ap[0] == 1.0 and first.tolist() == [1]
    _same(RR.rank_positives(S, [1, 1], gl), RR.brute_force(S, [1, 1], gl))
    _same(RR.rank_positives(S, [1, 1], gl2), RR.brute_force(S, [1, 1], gl2))


def test_lone_query_and_average_precision_order():
    S = np.array([[0.3, 0.9, 0.1, 0.7, 0.5],
                  [0.3, 0.9, 0.1, 0.7, 0.5]], dtype=np.float32)
    gl = np.array([7, 8, 7, 8, 7])
    off, idx, ranks, ap, first = RR.rank_positives(S, [7, 9], gl)
    assert off.tolist() == [0, 3, 3]
    assert idx.tolist() == [4, 0, 2] and ranks.tolist() == [3, 4, 5]
    assert ap[0] == (1.0 / 3.0 + 2.0 / 4.0 + 3.0 / 5.0) / 3.0           # added in rank order
    assert ap[1] == 0.0 and first.tolist() == [3, 0]                     # the lone query
    assert RR.cmc(first, np.diff(off), 3) == 1.0 and RR.cmc(first, np.diff(off), 2) == 0.0
    _same(RR.rank_positives(S, [7, 9], gl), RR.brute_force(S, [7, 9], gl))


def test_excluded_row_that_would_have_been_the_best_positive():
    S = np.array([[0.99, 0.2, 0.6, 0.4]], dtype=np.float32)
    gl = np.array([1, 0, 1, 0])
    off, idx, ranks, ap, first = RR.rank_positives(S, [1], gl)
    assert idx.tolist() == [0, 2] and ranks.tolist() == [1, 2]
    for offset in (0, 100):
        ex = np.array([0 + offset])
        off, idx, ranks, ap, first = RR.rank_positives(S, [1], gl, ex, offset)
        assert idx.tolist() == [2 + offset] and ranks.tolist() == [1] and first.tolist() == [1]
        _same(RR.rank_positives(S, [1], gl, ex, offset), RR.brute_force(S, [1], gl, ex, offset))
    # an excluded row of another shard (outside [idx_offset, idx_offset + G)) or a negative one excludes nothing
    for ex in (np.array([0]), np.array([-1]), np.array([104])):
        _same(RR.rank_positives(S, [1], gl, ex, 100), RR.rank_positives(S, [1], gl, None, 100))


def test_nan_and_signed_zero():
    nan = np.float32(np.nan)
    S = np.array([[0.5, nan, -0.0, 0.0, nan, 0.25]], dtype=np.float32)
    gl = np.array([0, 1, 0, 1, 0, 1])
    off, idx, ranks, ap, first = RR.rank_positives(S, [0], gl)
    assert idx.tolist() == [4, 0, 2] and ranks.tolist() == [2, 3, 5]     # NaN first (rows 1, 4), then 0.5, 0.25, -0 before +0
    _same(RR.rank_positives(S, [0], gl), RR.brute_force(S, [0], gl))
    _same(RR.rank_positives(S, [1], gl), RR.brute_force(S, [1], gl))


def test_random_matrices_with_many_ties_match_the_brute_force():
    rng = np.random.default_rng(5)
    for trial in range(6):
        Q, G = 7, 23
        S = rng.integers(-2, 3, (Q, G)).astype(np.float32) / 4
        S[rng.random((Q, G)) < 0.05] = np.nan
        ql, gl = rng.integers(0, 4, Q), rng.integers(0, 3, G)
        ex = rng.integers(-1, G, Q) + 50
        _same(RR.rank_positives(S, ql, gl, ex, 50), RR.brute_force(S, ql, gl, ex, 50))
