"""The exact selection reference (tests/select_ref.py) against torch.topk where torch defines the answer, and against
hand-written rows where the library's own rules (ties, NaN, missing candidates, pads) do.  No GPU."""
import numpy as np
import torch

import select_ref as R

INF, NAN = np.float32(np.inf), np.float32(np.nan)
PAD = R.IDX_PAD


def f32(rows):
    return np.array(rows, dtype=np.float32)


def test_matches_torch_topk_without_ties_or_nan():
    rng = np.random.default_rng(5)
    for n, k in ((8, 8), (257, 5), (5000, 150), (9000, 1024)):
        v = rng.permutation(n * 3).astype(np.float32).reshape(3, n) - np.float32(n)      # distinct in every row
        tv, ti = torch.topk(torch.from_numpy(v), k)
        gv, gi = R.select_topk(v, None, k)
        np.testing.assert_array_equal(gi, ti.numpy())
        np.testing.assert_array_equal(gv, tv.numpy())
        gv, gi = R.select_topk(v, None, k, idx_offset=2 ** 33)
        np.testing.assert_array_equal(gi, ti.numpy() + 2 ** 33)


def test_ties_go_to_the_lower_index_and_zeros_tie():
    v = f32([[1, 3, 3, -0.0, 0.0, 3, -1, 0.0]])
    gv, gi, pos = R.select_topk(v, None, 7, return_pos=True)
    assert gi.tolist() == [[1, 2, 5, 0, 3, 4, 7]]
    assert pos.tolist() == gi.tolist()
    assert R.bits(gv).tolist() == R.bits(f32([[3, 3, 3, 1, -0.0, 0.0, 0.0]])).tolist()    # the input's own bits: -0 stays -0
    # explicit indices: the index decides a tie, not the position
    idx = np.array([[70, 60, 50, 40, 30, 20, 10, 0]], np.int64)
    gv, gi = R.select_topk(v, idx, 4)
    assert gi.tolist() == [[20, 50, 60, 70]] and gv.tolist() == [[3, 3, 3, 1]]


def test_nan_is_the_largest_value_in_index_order():
    v = f32([[0.5, NAN, INF, -INF, NAN, 2, NAN, -INF]])
    gv, gi = R.select_topk(v, None, 8)
    assert gi.tolist() == [[1, 4, 6, 2, 5, 0, 3, 7]]
    assert np.isnan(gv[0, :3]).all() and gv[0, 3:].tolist() == [INF, 2, 0.5, -INF, -INF]
    gv, gi = R.select_topk(v, None, 2)                    # more NaNs than k
    assert gi.tolist() == [[1, 4]] and np.isnan(gv).all()


def test_missing_candidates_never_take_a_slot():
    v = f32([[9, -INF, 7, NAN, -INF, 8, 1, 5]])
    idx = np.array([[PAD, 4, 2 ** 40, PAD, 3, 2 ** 62, 6, PAD]], np.int64)      # 9, NaN, 8 and 5 are no candidates
    gv, gi, pos = R.select_topk(v, idx, 6, return_pos=True)
    assert gi.tolist() == [[2 ** 40, 6, 3, 4, PAD, PAD]]                        # a real -inf beats an empty slot
    assert gv.tolist() == [[7, 1, -INF, -INF, -INF, -INF]]
    assert pos.tolist() == [[2, 6, 4, 1, -1, -1]]


def test_filtered_selection_and_pads():
    v = f32([[5, 4, 3, 2, 1, 0, 6, 7], [5, 4, 3, 2, 1, 0, 6, 7]])
    glab = np.array([1, 1, 2, 2, 1, 3, 2, 1], np.int64)
    qlab = np.array([1, 3], np.int64)
    ex = np.array([107, -1], np.int64)
    gv, gi = R.select_filtered(v, 4, 100, ex, qlab, glab, R.LABEL_SAME)
    assert gi.tolist() == [[100, 101, 104, -1], [105, -1, -1, -1]]
    assert gv.tolist() == [[5, 4, 1, -INF], [0, -INF, -INF, -INF]]
    gv, gi = R.select_filtered(v, 3, 100, ex, qlab, glab, R.LABEL_DIFFERENT)
    assert gi.tolist() == [[106, 102, 103], [107, 106, 100]]
    gv, gi = R.select_filtered(v, 2, 100, ex)
    assert gi.tolist() == [[106, 100], [107, 106]]


def test_pack_unpack_merge():
    odd_nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    v = f32([[odd_nan, -0.0], [1.5, -INF]])
    i = np.array([[3, 0], [2, 1]], np.int64)
    p = R.pack(v, i, 2, 3)
    assert p.view(np.uint32).tolist() == [[[0x7FC12345, 3], [0x80000000, 0], [0xFF800000, 0xFFFFFFFF]],
                                          [[0x3FC00000, 2], [0xFF800000, 1], [0xFF800000, 0xFFFFFFFF]]]
    empty = R.pack(None, None, 2, 3)
    assert (empty.view(np.uint32) == np.array([0xFF800000, 0xFFFFFFFF], np.uint32)).all()
    cv, ci = R.unpack(np.stack([p, empty]), [2 ** 33, 7])
    assert ci.tolist() == [[2 ** 33 + 3, 2 ** 33, 2 ** 62, 2 ** 62, 2 ** 62, 2 ** 62],
                           [2 ** 33 + 2, 2 ** 33 + 1, 2 ** 62, 2 ** 62, 2 ** 62, 2 ** 62]]
    gv, gi = R.unpack_merge(np.stack([p, empty]), [2 ** 33, 7], 3)
    assert gi.tolist() == [[2 ** 33 + 3, 2 ** 33, PAD], [2 ** 33 + 2, 2 ** 33 + 1, PAD]]
    assert R.bits(gv).tolist() == [[0x7FC12345, 0x80000000, 0xFF800000], [0x3FC00000, 0xFF800000, 0xFF800000]]
    cv, ci = R.clear_pads(gv, gi, 0, 2 ** 34)
    assert ci.tolist() == [[2 ** 33 + 3, 2 ** 33, -1], [2 ** 33 + 2, 2 ** 33 + 1, -1]]


def test_hit_counts_and_distinct_classes_skip_pads():
    gcls = np.array([5, 5, 2 ** 40, 7, 5], np.int64)
    idx = np.array([[-1, 0, 5, 3], [PAD, 5, -1, 0], [2, 2, 3, 1], [3, -1, 0, 4]], np.int64)
    qcls = np.array([5, 5, 2 ** 40, 5], np.int64)
    assert R.hit_counts(idx, qcls, gcls) == (1, 3)           # top-1: row 2 only; top-3: rows 0, 2, 3 (row 1's hit is 4th)
    val = np.arange(16, dtype=np.float32).reshape(4, 4)
    oc, oi, ov = R.distinct_topn(idx, val, gcls, 3)
    assert oc.tolist() == [[5, 7, -1], [5, -1, -1], [2 ** 40, 7, 5], [7, 5, -1]]
    assert oi.tolist() == [[0, 3, -1], [0, -1, -1], [2, 3, 1], [3, 0, -1]]
    np.testing.assert_array_equal(ov, f32([[1, 3, NAN], [7, NAN, NAN], [8, 10, 11], [12, 14, NAN]]))
