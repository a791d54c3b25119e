"""Alpha query expansion / DBA without a GPU: argument errors of mi355_expand_rows and of the Python API, the float64 reference
against a hand-worked example, and the tolerance of the GPU tests against the bugs it must catch."""
import math

import numpy as np
import pytest
import torch

import qe_ref
from imageretrievalresearch_amd import MI355Error, _lib
from imageretrievalresearch_amd import rank as R

F32, F16 = _lib.DTYPE_F32, _lib.DTYPE_F16


def _call(base=1, base_dtype=F32, base_ld=8, norm=1, gallery=1, gallery_dtype=F32, G=10, gld=8, dim=8, vals=1, idx=1, rows=4,
          n=3, off=0, alpha=3.0, eps=1e-6, out=16, out_dtype=F32, out_ld=8, ws=None, ws_bytes=0):
    L = _lib.lib()
    return L.mi355_expand_rows(base, base_dtype, base_ld, norm, gallery, gallery_dtype, G, gld, dim, vals, idx, rows, n, off,
                               alpha, eps, out, out_dtype, out_ld, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(base=None), b"null"), (dict(gallery=None), b"null"), (dict(vals=None), b"null"), (dict(idx=None), b"null"),
    (dict(out=None), b"null"),
    (dict(n=0), b"n=0"), (dict(alpha=-1.0), b"alpha"), (dict(alpha=math.nan), b"alpha"), (dict(alpha=math.inf), b"alpha"),
    (dict(base_ld=7), b"leading dims"), (dict(gld=4), b"leading dims"), (dict(out_ld=5), b"leading dims"),
    (dict(dim=0), b"bad shape"), (dict(rows=-1), b"bad shape"), (dict(base_dtype=7), b"dtype"),
    (dict(norm=1, base_dtype=F16), b"normalize_base"), (dict(out=8), b"aligned"), (dict(out_ld=10), b"aligned"),
    (dict(out_dtype=F16), b"workspace"),
])
def test_expand_rows_rejects_bad_arguments_before_any_hip_call(kw, msg):
    assert _call(**kw) != 0
    assert msg in _lib.lib().mi355_last_error(), (kw, _lib.lib().mi355_last_error())


def test_expand_workspace_bytes():
    L = _lib.lib()
    assert L.mi355_expand_workspace_bytes(256, 1536, F32) == 0
    assert L.mi355_expand_workspace_bytes(256, 1536, F16) == 256 * 1536 * 4
    assert L.mi355_expand_workspace_bytes(0, 1536, F16) == 0
    assert _call(rows=0) == 0                          # R = 0 does nothing (no HIP call)


def test_python_api_rejects_cpu_tensors_and_bad_qe():
    q, g = torch.randn(4, 8), torch.randn(10, 8)
    with pytest.raises(MI355Error, match="GPU"):
        R.expand_queries(q, g, 2)
    for bad in [(0, 3.0), (2, -1.0), (2, float("nan")), (2, float("inf")), (2.5, 1.0), (True, 1.0)]:
        with pytest.raises(MI355Error):
            R.expand_queries(q, g, *bad)
    gal = R.Gallery(8, "cpu")
    for qe in [3, (3,), (3, 1.0, 2), "ab", (0, 1.0), (3, -0.5)]:
        with pytest.raises(MI355Error):
            gal.search(q, 1, qe=qe)
    with pytest.raises(MI355Error):
        gal.expand_queries(q, 2, 1.0)                  # CPU queries
    with pytest.raises(MI355Error):
        gal.augmented(0)
    with pytest.raises(MI355Error):
        R.retrieval_accuracy(torch.randn(4, 8), torch.zeros(4, dtype=torch.int64), query_expansion=(2, 1.0))


def test_reference_matches_a_hand_worked_example():
    # q = (3, 4) -> qn = (0.6, 0.8); rows e1, e2, (1, 1)/sqrt2; slots: (0.5, 0) (0.25, 1) (-inf, -1) (-0.2, 2) (nan, 2)
    rows = np.array([[1.0, 0.0], [0.0, 1.0], [np.sqrt(0.5), np.sqrt(0.5)]])
    vals = np.array([[0.5, 0.25, -np.inf, -0.2, np.nan]])
    idx = np.array([[0, 1, -1, 2, 2]])
    x = qe_ref.expand_sum(np.array([[3.0, 4.0]]), rows, vals, idx, alpha=2.0)
    np.testing.assert_allclose(x, [[0.6 + 0.25, 0.8 + 0.0625]], rtol=0, atol=1e-15)
    out = qe_ref.expand(np.array([[3.0, 4.0]]), rows, vals, idx, alpha=2.0)
    np.testing.assert_allclose(out, [[0.85, 0.8625]] / np.hypot(0.85, 0.8625), rtol=0, atol=1e-15)
    # alpha = 0: every used slot weighs 1 (average QE); a NaN row behind a skipped slot stays out
    rows_nan = rows.copy()
    rows_nan[2] = np.nan
    x0 = qe_ref.expand_sum(np.array([[3.0, 4.0]]), rows_nan, vals, idx, alpha=0.0)
    np.testing.assert_allclose(x0, [[1.6, 1.8]], rtol=0, atol=1e-15)
    # DBA form: the base as it is (not renormalised); idx_offset shifts the global indices
    xd = qe_ref.expand_sum(np.array([[1.0, 0.0]]), rows, np.array([[0.5]]), np.array([[11]]), 1.0, normalize_base=False,
                           idx_offset=10)
    np.testing.assert_allclose(xd, [[1.0, 0.5]], rtol=0, atol=1e-15)


def tolerance(n):
    """The per-row L2 bound of tests/test_query_expansion_gpu.py (kept in one place)."""
    return max(4e-6, (n + 2) * 2.0 ** -23)


@pytest.mark.parametrize("n", [1, 10, 64])
@pytest.mark.parametrize("D", [70, 1536])
def test_the_gpu_tolerance_sits_far_below_the_bugs_it_must_catch(n, D):
    """On the GPU test's shapes (its data generator), each bug moves every affected row by more than 10x the tolerance."""
    q, g, vals, idx, pads = qe_ref.kernel_case(D, n, seed=D + n)
    gn = qe_ref.normalize(g)
    good = qe_ref.expand(q, gn, vals, idx, 3.0)
    tol = 10 * tolerance(n)

    def moved(bad, rows=slice(None)):
        d = np.sqrt(((bad - good) ** 2).sum(1))[rows]
        assert d.min() > tol, (d.min(), tol)

    # dropping the base row
    moved(qe_ref.normalize(qe_ref.expand_sum(q, gn, vals, idx, 3.0) - qe_ref.normalize(q)))
    # score instead of score ** alpha (rows with a used slot)
    used = qe_ref.slot_weights(vals, idx, 3.0, g.shape[0])[2].any(1)
    moved(qe_ref.expand(q, gn, vals, idx, 1.0), used)
    # counting a pad slot (weight 1 on row 0)
    cnt = np.where(np.isneginf(vals), 1.0, vals)
    moved(qe_ref.expand(q, gn, cnt, np.where(idx < 0, 0, idx), 3.0), pads)
    # not normalising the query
    moved(qe_ref.normalize(qe_ref.expand_sum(q, gn, vals, idx, 3.0, normalize_base=False)), used)
