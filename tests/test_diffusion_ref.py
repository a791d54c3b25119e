"""The NumPy model of diffusion re-ranking (tests/diffusion_ref.py) against its own invariants, without a GPU: S is symmetric with
spectral radius <= 1, the float64 CG equals a direct solve, diffusion helps on the arcs fixture, and the premise of the GPU
tests' index check (few near-ties in the model's top 10) holds on the cases those tests name."""
import functools

import numpy as np
import pytest

import diffusion_ref as dr
from imageretrievalresearch_amd import diffusion  # noqa: F401  (the feature under test: these tests belong to it)

Q = 37
# (L, kd, kq, iters): the solve cases of tests/test_diffusion_gpu.py
CASES = [(64, 8, 5, 20), (257, 32, 5, 20), (257, 32, 5, 64), (1024, 32, 10, 20), (1024, 16, 1024, 64), (480, 5, 1, 1), (64, 1, 5, 20)]
INDEX_CASES = CASES[:4]
ALPHA, GAMMA = 0.99, 3


@functools.lru_cache(maxsize=None)
def _arcs(narcs):
    rows, labels = dr.arcs(narcs)
    q, own, ql = dr.arc_queries(rows, narcs, 40, Q)
    return rows, labels, q, own, ql


@functools.lru_cache(maxsize=None)
def _index(narcs, kd, gamma=GAMMA):
    rows = _arcs(narcs)[0]
    nv, nn = dr.knn(rows, rows, kd, np.arange(len(rows)))
    return dr.graph(nn, nv, gamma)


@functools.lru_cache(maxsize=None)
def _case(L, kd, kq, iters):
    narcs = 30 if L > 480 else 12
    rows, _, q, own, _ = _arcs(narcs)
    cols, vals, _ = _index(narcs, kd)
    sv, si = dr.knn(q, rows, L, own)
    y = dr.source(sv, si, kq, GAMMA)
    return cols, vals, si, y, dr.solve(cols, vals, si, y, ALPHA, iters)


@pytest.mark.parametrize("kd, gamma", [(1, 1), (5, 3), (10, 3), (32, 1), (32, 3)])
def test_s_is_symmetric_with_spectral_radius_at_most_one(kd, gamma):
    cols, vals, deg = _index(12, kd, gamma)
    S = dr.dense(cols, vals)
    assert np.array_equal(S, S.T)
    assert np.abs(np.linalg.eigvalsh(S)).max() <= 1 + 1e-12
    assert ((cols >= 0) | (vals == 0)).all() and (deg >= 0).all()
    # the same in fp32: the two directions of an edge hold the same bits
    c32, v32, _ = dr.graph(*reversed(dr.knn(_arcs(12)[0], _arcs(12)[0], kd, np.arange(480))), gamma, np.float32)
    S32 = dr.dense(c32, v32)
    assert v32.dtype == np.float32 and np.array_equal(c32, cols) and np.array_equal(S32, S32.T)


@pytest.mark.parametrize("L, kd, kq, iters", [c for c in CASES if c[0] <= 257])
def test_cg_equals_a_direct_solve(L, kd, kq, iters):
    cols, vals, si, y, _ = _case(L, kd, kq, 64)
    f, its = dr.solve(cols, vals, si, y, ALPHA, 64)
    worst = 0.0
    for q in range(Q):
        want = dr.direct(cols, vals, si[q], y[q], ALPHA)
        worst = max(worst, np.abs(f[q] - want).max() / np.abs(want).max())
    print(f"L={L} kd={kd}: CG at <= 64 iterations vs np.linalg.solve: {worst:.2e} relative, {its.min()}..{its.max()} iterations")
    assert worst <= 1e-6


def test_cg_stays_finite_and_freezes():
    cols, vals, si, y, (f, its) = _case(1024, 16, 1024, 64)
    assert np.isfinite(f).all() and (its >= 1).all()
    f32, its32 = dr.solve(cols, vals, si[:4], y[:4], ALPHA, 64, np.float32)
    assert np.isfinite(f32).all()
    print(f"L=1024 kd=16: float64 stops at {its.min()}..{its.max()} of 64, fp32 at {its32.min()}..{its32.max()}")
    # y = 0: no iteration, f = 0
    f0, it0 = dr.solve(cols, vals, si[:1], np.zeros_like(y[:1]), ALPHA, 20)
    assert it0[0] == 0 and (f0 == 0).all()


def test_diffusion_follows_the_arcs():
    rows, labels, q, own, ql = _arcs(12)
    plain = dr.knn(q, rows, 200, own)[1]
    _, ranked = dr.diffuse(rows, q, 200, kd=10, kq=5, alpha=ALPHA, gamma=GAMMA, iters=20, L=200, exclude=own)
    before, after = dr.r_precision(plain, labels, ql, own), dr.r_precision(ranked, labels, ql, own)
    print(f"arcs R-precision: plain {before:.3f}, diffusion {after:.3f}")
    assert after >= before + 0.05


@pytest.mark.parametrize("L, kd, kq, iters", INDEX_CASES)
def test_few_near_ties_in_the_top_ten(L, kd, kq, iters):
    f = _case(L, kd, kq, iters)[4][0]
    close = dr.close_pairs(f, 10)
    print(f"L={L} kd={kd} kq={kq} iters={iters}: {int(close.sum())} of {close.size} top-10 positions next to a near-tie")
    assert close.mean() <= 0.05
