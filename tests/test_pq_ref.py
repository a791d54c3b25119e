"""The NumPy model of the product-quantised gallery (pq_ref.py) against cases worked out by hand, and Lloyd's descent on a
seeded clustered input: what the GPU tests compare against is itself checked here, without a GPU."""
import numpy as np

import pq_ref as R

F32 = np.float32


def _grid_codebooks(M):
    """dsub = 1: centroid c of every sub-quantiser is (c - 128) / 128, exact in fp32."""
    cb = ((np.arange(256, dtype=np.float64) - 128.0) / 128.0).astype(F32)
    return np.ascontiguousarray(np.broadcast_to(cb[None, :, None], (M, 256, 1)))


def test_dsub_1_picks_the_nearest_grid_point():
    cb = _grid_codebooks(4)
    n = np.array([[0.5, -0.25, 0.0, 127.0 / 128.0],          # on the grid: distance 0
                  [0.501, -1.5, 0.0039, 2.0]], F32)          # nearest: 192, 0 (the lowest point), 128 (0.0039 < 1/256), 255
    assert R.encode(n, cb).tolist() == [[192, 96, 128, 255], [192, 0, 128, 255]]


def test_an_exact_tie_goes_to_the_lower_centroid():
    cb = np.full((4, 256, 1), 100.0, F32)
    cb[:, 20, 0] = 0.75                                      # (0.5 - 0.75)^2 == (0.5 - 0.25)^2 == 0.0625 exactly
    cb[:, 10, 0] = 0.25
    cb[2, 5, 0] = 0.75                                       # subspace 2: the tie is between 5 and 10
    n = np.full((1, 4), 0.5, F32)
    assert R.encode(n, cb).tolist() == [[10, 10, 5, 10]]


def test_a_nan_element_gives_code_0_in_its_subspace_only():
    cb = np.zeros((4, 256, 2), F32)
    cb[:, :, 0] = ((np.arange(256) - 128.0) / 128.0).astype(F32)[None, :]
    n = np.array([[0.5, 0.0, np.nan, 0.0, 0.25, 0.0, 0.0, np.nan]], F32)
    assert R.encode(n, cb).tolist() == [[192, 0, 160, 0]]


def test_the_table_is_a_rounded_product_then_a_rounded_add():
    # x * b = 1 + 2^-11 + 2^-24 exactly; rounded to fp32 it is 1 + 2^-11 (the tie goes to the even neighbour), and adding
    # -(1 + 2^-11) gives 0.  One fused multiply-add would keep the 2^-24.
    x = F32(1.0 + 2.0 ** -12)
    cb = np.zeros((4, 256, 2), F32)
    cb[0, 7] = [x, 1.0]
    qn = np.zeros((1, 8), F32)
    qn[0, :2] = [x, -(1.0 + 2.0 ** -11)]
    T = R.table(qn, cb)
    assert T.shape == (1, 4, 256) and T[0, 0, 7] == 0.0
    assert float(np.float64(x) * np.float64(x) - (1.0 + 2.0 ** -11)) == 2.0 ** -24


def test_the_score_adds_into_four_accumulators():
    vals = [1e8, 1.0, -1e8, 1.0, 1.0, 1.0, 1.0, 1.0]         # m = 0 .. 7
    codes = np.array([[3, 1, 4, 1, 5, 9, 2, 6]], np.uint8)
    T = np.zeros((1, 8, 256), F32)
    for m, v in enumerate(vals):
        T[0, m, codes[0, m]] = v
    # a0 = 1e8 + 1 = 1e8, a1 = 2, a2 = -1e8 + 1 = -1e8, a3 = 2 (fp32: the spacing at 1e8 is 8); (1e8 + 2) + (-1e8 + 2) = 0
    assert R.scores(T, codes)[0, 0] == 0.0
    seq = F32(0)
    for v in vals:
        seq = F32(seq + F32(v))
    assert seq == 5.0                                         # the sequential sum is another number


def test_update_is_the_float64_mean_and_keeps_empty_cells():
    cb = np.zeros((4, 256, 1), F32)
    cb[:, :, 0] = np.arange(256, dtype=F32)[None, :]
    n = np.array([[1, 0, 0, 0], [2, 0, 0, 0], [4, 0, 0, 0]], F32)
    codes = np.array([[9, 0, 0, 0], [9, 0, 0, 1], [7, 0, 0, 1]], np.uint8)
    out, counts = R.update(n, codes, cb)
    assert out[0, 9, 0] == 1.5 and out[0, 7, 0] == 4.0 and out[0, 8, 0] == 8.0      # cell 8 is empty: unchanged
    assert counts[0, 9] == 2 and counts[0, 7] == 1 and counts[3, 1] == 2 and counts.sum() == 12


def test_topk_with_a_mask_pads_with_minus_one():
    s = np.array([[0.5, np.nan, 0.5, -0.0, 0.0]], F32)
    v, i = R.topk(s, 4)
    assert i.tolist() == [[1, 0, 2, 3]] and np.isnan(v[0, 0])
    v, i = R.topk(s, 4, np.array([[True, False, True, False, True]]))
    assert i.tolist() == [[0, 2, 4, -1]] and v[0, 3] == -np.inf


def test_lloyd_descends_on_clustered_rows():
    n = R.clustered_rows(4096, 64, 40, 0.3, seed=0)
    pick = np.random.RandomState(1).permutation(4096)[:256]
    _, dist = R.lloyd(n, 8, 5, pick)
    print("distortion:", " -> ".join(f"{d:.4f}" for d in dist))
    assert len(dist) == 6
    assert all(b < a for a, b in zip(dist, dist[1:])), dist
