"""Feature-map aggregation without a GPU: the R-MAC region grid of the package against literal lists and against the exact
restatement of tests/aggregate_ref.py, sanity checks of the float64 model the GPU tests compare with, and the planted-patch
fixture that shows why the feature exists - GeM and R-MAC find the class a mean over positions loses."""
import numpy as np
import pytest

import aggregate_ref as A
from imageretrievalresearch_amd import MI355Error, rmac_regions

GRID_7x7 = ([(0, 0, 7, 7)] + [(y, x, 4, 4) for y in (0, 3) for x in (0, 3)]
            + [(y, x, 3, 3) for y in (0, 2, 4) for x in (0, 2, 4)])
GRID_7x10 = ([(0, 0, 7, 7), (0, 3, 7, 7)] + [(y, x, 4, 4) for y in (0, 3) for x in (0, 3, 6)]
             + [(y, x, 3, 3) for y in (0, 2, 4) for x in (0, 2, 4, 7)])


def _grid(H, W, levels=3):
    t = rmac_regions(H, W, levels)
    assert t.dtype.is_floating_point is False and str(t.dtype) == "torch.int32" and t.dim() == 2 and t.shape[1] == 4 and not t.is_cuda
    return [tuple(r) for r in t.tolist()]


def test_the_literal_grids():
    assert _grid(7, 7) == GRID_7x7 and len(GRID_7x7) == 14
    assert _grid(7, 10) == GRID_7x10 and len(GRID_7x10) == 20
    assert _grid(10, 7) == [(x, y, w, h) for (y, x, h, w) in _transpose_order(GRID_7x10)]
    assert _grid(1, 1) == [(0, 0, 1, 1)]
    assert len(_grid(32, 32)) == 14 and len(_grid(17, 33)) == 26
    assert A.rmac_regions(7, 7) == GRID_7x7 and A.rmac_regions(7, 10) == GRID_7x10


def _transpose_order(grid):
    """The regions of a W x H grid listed in the order their transposes appear on the H x W map (rows outer, columns inner)."""
    out, i = [], 0
    while i < len(grid):
        side = grid[i][2]
        level = [g for g in grid if g[2] == side]
        out += sorted(level, key=lambda g: (g[1], g[0]))
        i += len(level)
    return out


def test_duplicates_are_kept_on_tiny_maps():
    g = _grid(2, 2)
    assert len(g) == 14 and len(set(g)) < 14


@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_every_region_lies_inside_the_map_and_both_statements_agree(levels):
    for H in range(1, 65):
        for W in range(1, 65):
            g = _grid(H, W, levels)
            assert g == A.rmac_regions(H, W, levels), (H, W, levels)
            assert g and all(h >= 1 and w >= 1 and y >= 0 and x >= 0 and y + h <= H and x + w <= W for y, x, h, w in g), (H, W)


def test_grid_arguments():
    for bad in ((0, 7), (7, 65), (7.0, 7), (True, 7)):
        with pytest.raises(MI355Error):
            rmac_regions(*bad)
    with pytest.raises(MI355Error):
        rmac_regions(7, 7, 0)
    with pytest.raises(MI355Error):
        rmac_regions(7, 7, 3, float("nan"))


# ---------------------------------------------------------------------------------------------- the model
def test_gem_at_p_1_is_the_clamped_mean():
    x = A.silu_map(3, (2, 5, 7, 7)).astype(np.float64)
    got = A.aggregate(x, "gem", p=1.0, normalize=False)
    np.testing.assert_allclose(got, np.maximum(x, 1e-6).mean(axis=(2, 3)), rtol=1e-13, atol=0)


def test_gem_tends_to_the_maximum_and_spoc_is_the_mean():
    x = np.abs(A.silu_map(4, (2, 5, 7, 7)).astype(np.float64)) + 0.1
    mx = x.max(axis=(2, 3))
    g64 = A.aggregate(x, "gem", p=64.0, normalize=False)
    assert (g64 <= mx * (1 + 1e-12)).all() and (g64 >= mx * 49 ** (-1 / 64.0) * (1 - 1e-12)).all()
    np.testing.assert_allclose(A.aggregate(x, "spoc", normalize=False), x.mean(axis=(2, 3)), rtol=1e-13)


def test_rmac_with_one_level_on_a_square_map_is_normalised_mac():
    x = A.silu_map(5, (3, 9, 7, 7))
    np.testing.assert_allclose(A.aggregate(x, "rmac", levels=1), A.aggregate(x, "mac"), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(A.aggregate(x, "rmac", levels=1)[0]), 1.0, rtol=1e-12)


def test_p_64_on_values_of_1e3_is_finite():
    x = np.full((1, 4, 7, 7), 1e3) * (1 + 0.1 * np.random.default_rng(0).random((1, 4, 7, 7)))
    g = A.aggregate(x, "gem", p=64.0, normalize=False)
    assert np.isfinite(g).all() and (g > 1e3 * 0.9).all() and (g <= x.max(axis=(2, 3))).all()
    assert np.isfinite(A.aggregate(x.astype(np.float32), "gem", p=64.0)).all()


def test_an_all_zero_map_gives_zeros_never_nan():
    z = np.zeros((1, 6, 7, 7), dtype=np.float32)
    for method in ("spoc", "mac", "rmac", "crow"):
        assert (A.aggregate(z, method) == 0).all(), method
    g = A.aggregate(z, "gem")                                       # the clamp lifts every channel to 1e-6: a constant unit vector
    np.testing.assert_allclose(g, np.full((1, 6), 6 ** -0.5), rtol=1e-12)


def test_crow_ignores_a_channel_that_is_never_positive_and_weights_rare_channels_up():
    x = A.silu_map(6, (2, 12, 7, 7))
    d = A.crow(x, normalize=False)
    assert (d[:, 0] == 0).all() and (d[-1] == 0).all()             # channel 0 is negative everywhere, the last image all zero
    y = np.zeros((1, 2, 2, 2))
    y[0, 0] = 1.0                                                   # on at 4 of 4 positions
    y[0, 1, 0, 0] = 1.0                                             # on at 1 of 4
    Q = np.array([1.0, 0.25])
    S = y[0].sum(axis=0)
    St = np.sqrt(S / np.sqrt((S * S).sum()))
    want = np.log(Q.sum() / Q) * np.array([(St * y[0, 0]).sum(), (St * y[0, 1]).sum()])
    np.testing.assert_allclose(A.crow(y, normalize=False)[0], want, rtol=1e-13)


# ---------------------------------------------------------------------------------------------- why the feature exists
def test_gem_and_rmac_find_the_planted_class_that_the_mean_loses():
    p1 = {}
    for method, kw in A.FIXTURE_METHODS:
        top, gap, p1[method, kw.get("pool")] = A.fixture_reference(method, kw)
        assert gap.min() > 1e-4, (method, kw, gap.min())            # no near-ties: the GPU test may compare top-1 exactly
    print("precision@1 of the float64 model:", p1)
    assert p1["spoc", None] < 0.6
    assert p1["gem", None] >= p1["spoc", None] + 0.3
    assert p1["rmac", None] >= p1["spoc", None] + 0.3
