"""The NumPy model of the binary gallery (binary_ref.py) against first principles, and the two conditions under which the
format is usable at all, on a planted mixture: with the column mean as centre a refined shortlist finds the float neighbours;
with a zero centre on pooled (all-positive) rows it finds nothing.  The two bounds are conditions on the inputs, not
measurements: >= 0.95 and <= 0.10 (the model gives 1.00 and about 0.03)."""
import numpy as np
import pytest

import binary_ref as R

DIMS = [1, 31, 32, 33, 96, 128, 130, 1000]


@pytest.mark.parametrize("dim", DIMS)
def test_distance_is_the_count_of_differing_signs(dim):
    r = np.random.default_rng(dim)
    g, q = R.normalize(r.standard_normal((70, dim))), R.normalize(r.standard_normal((9, dim)))
    c = (0.1 * r.standard_normal(dim) / np.sqrt(dim)).astype(np.float32)
    g[4, 0] = np.nan                                                  # a NaN: bit 0
    for center in (None, c):
        cc = np.zeros(dim, np.float32) if center is None else center
        g[3, dim // 2] = cc[dim // 2]                                 # an element exactly at the centre: bit 1
        gc, qc = R.encode(g, center), R.encode(q, center)
        assert gc.dtype == np.uint32 and gc.shape == (70, R.words(dim))
        with np.errstate(invalid="ignore"):
            sg, sq = np.where(g >= cc, 1, -1), np.where(q >= cc, 1, -1)
        bit = lambda codes, i, j: int(codes[i, j // 32] >> np.uint32(j % 32)) & 1   # noqa: E731
        assert bit(gc, 3, dim // 2) == 1 and bit(gc, 4, 0) == 0
        for j in range(dim):
            assert bit(gc, 0, j) == (sg[0, j] > 0)
        if dim % 32:                                                  # pad bits of the last word
            assert (gc[:, -1] >> np.uint32(dim % 32) == 0).all()
        d = R.distances(qc, gc)
        brute = (sq[:, None, :] != sg[None, :, :]).sum(axis=2)
        assert d.dtype == np.int32 and (d == brute).all() and d.min() >= 0 and d.max() <= dim
        # the score is the cosine of the two +-1 vectors: their exact dot over dim (53 bits hold the quotient's double
        # rounding harmless: 53 >= 2 * 24 + 2)
        s = R.scores(d, dim)
        dot = (sq[:, None, :] * sg[None, :, :]).sum(axis=2)
        assert s.dtype == np.float32 and (s == (dot.astype(np.float64) / dim).astype(np.float32)).all()


def test_nan_queries_and_selection_order():
    dim = 40
    r = np.random.default_rng(7)
    g, q = R.normalize(r.standard_normal((50, dim))), R.normalize(r.standard_normal((3, dim)))
    q[1, 5] = np.nan
    g = np.concatenate([g, g])                                        # every row twice: ties
    d = R.distances(R.encode(q), R.encode(g), R.has_nan(q))
    assert (d[1] == -1).all() and (d[0] >= 0).all()
    s = R.scores(d, dim)
    assert np.isnan(s[1]).all() and not np.isnan(s[0]).any()
    v, i = R.select(s, 100)
    assert (i[1] == np.arange(100)).all() and np.isnan(v[1]).all()    # all NaN: the rows in order
    assert (np.diff(v[0]) <= 0).all()
    same = np.diff(v[0]) == 0
    assert same.any() and (np.diff(i[0])[same] > 0).all()             # ties to the lower row
    mask = np.zeros((3, 100), bool)
    mask[:, [7, 57, 9]] = True
    v, i = R.select(s, 5, mask)
    assert sorted(i[0, :3].tolist()) == [7, 9, 57] and (i[:, 3:] == -1).all() and np.isneginf(v[:, 3:]).all()
    assert list(i[0, :2]) == [7, 57] or s[0, 9] > s[0, 7]             # rows 7 and 57 are the same row: 7 first


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_centre_decides_whether_the_format_works(seed):
    x, q = R.planted_mixture(seed)
    for rows, queries in ((x, q), (R.pooled(x), R.pooled(q))):
        n, qn = R.normalize(rows), R.normalize(queries)
        c = R.mean_center(n)
        got = R.refined_recall(n, qn, R.encode(n, c), R.encode(qn, c))
        print(f"seed {seed}: mean centre, refined recall@10 at a shortlist of 100: {got:.4f}")
        assert got >= 0.95
    zero = R.refined_recall(n, qn, R.encode(n), R.encode(qn))         # the pooled rows, raw signs
    print(f"seed {seed}: zero centre on pooled rows: {zero:.4f}")
    assert zero <= 0.10
    assert (R.encode(n) == R.encode(np.ones_like(n))).all()           # every sign bit is set: the codes carry nothing
