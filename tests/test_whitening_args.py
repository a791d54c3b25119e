"""PCA whitening without a GPU: argument errors of mi355_embedding_moments / mi355_whiten_rows (before any HIP call), and
Whitening.from_moments - all host float64 - against the numpy reference of tests/whiten_ref.py."""
import numpy as np
import pytest
import torch

import whiten_ref
import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import MI355Error, Whitening, _lib

F32, F16 = _lib.DTYPE_F32, _lib.DTYPE_F16


def _moments(rows=1, dtype=F32, R=4, ld=8, dim=8, norm=0, eps=1e-6, acc=0, s=8, o=16, ws=16, ws_bytes=None):
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = L.mi355_moments_workspace_bytes(R, dim)
    return L.mi355_embedding_moments(rows, dtype, R, ld, dim, norm, eps, acc, s, o, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(rows=None), b"null"), (dict(s=None), b"null"), (dict(o=None), b"null"),
    (dict(dim=0), b"bad shape"), (dict(R=-1), b"bad shape"), (dict(ld=7), b"leading dim"),
    (dict(dtype=5), b"dtype"), (dict(dtype=F16, norm=1), b"normalize_rows"), (dict(eps=float("nan")), b"eps"),
    (dict(ws=None), b"workspace"), (dict(ws=8), b"workspace"), (dict(ws_bytes=16), b"workspace"),
])
def test_embedding_moments_rejects_bad_arguments_before_any_hip_call(kw, msg):
    assert _moments(**kw) != 0
    assert msg in _lib.lib().mi355_last_error(), (kw, _lib.lib().mi355_last_error())


def _whiten(x=16, x_dtype=F32, R=4, x_ld=8, din=8, norm_in=1, eps=1e-6, mat=16, bias=16, dout=4, norm_out=1, out=16, out_dtype=F32,
            out_ld=4, ws=None, ws_bytes=0):
    L = _lib.lib()
    return L.mi355_whiten_rows(x, x_dtype, R, x_ld, din, norm_in, eps, mat, bias, dout, norm_out, out, out_dtype, out_ld, ws,
                               ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(x=None), b"null"), (dict(mat=None), b"null"), (dict(bias=None), b"null"), (dict(out=None), b"null"),
    (dict(din=0, dout=0), b"bad shape"), (dict(R=-1), b"bad shape"), (dict(dout=0), b"dim_out"), (dict(dout=9, out_ld=12), b"dim_out"),
    (dict(x_ld=7), b"leading dims"), (dict(out_ld=3), b"leading dims"),
    (dict(x_dtype=3), b"dtype"), (dict(out_dtype=9), b"dtype"),
    (dict(x_dtype=F16, norm_in=1), b"normalize_input"), (dict(out_dtype=F16, norm_out=0), b"normalize_output"),
    (dict(out=8), b"aligned"), (dict(out_ld=6), b"aligned"), (dict(eps=-1.0), b"eps"),
    (dict(out_dtype=F16, out_ld=64), b"workspace"), (dict(out_dtype=F16, out_ld=64, ws=16, ws_bytes=8), b"workspace"),
])
def test_whiten_rows_rejects_bad_arguments_before_any_hip_call(kw, msg):
    assert _whiten(**kw) != 0
    assert msg in _lib.lib().mi355_last_error(), (kw, _lib.lib().mi355_last_error())


def test_workspace_sizes_and_empty_calls():
    L = _lib.lib()
    assert L.mi355_moments_workspace_bytes(0, 1536) == 0
    assert L.mi355_moments_workspace_bytes(100000, 1536) > 0
    # the split is a function of (R, dim) alone: asking twice gives the same size, and more rows never need less
    assert L.mi355_moments_workspace_bytes(4099, 70) == L.mi355_moments_workspace_bytes(4099, 70)
    assert L.mi355_moments_workspace_bytes(200000, 64) >= L.mi355_moments_workspace_bytes(1000, 64)
    assert L.mi355_whiten_workspace_bytes(0, 1536, 256, F16) == 0
    assert L.mi355_whiten_workspace_bytes(100, 1536, 256, F32) == 0
    assert L.mi355_whiten_workspace_bytes(100, 1536, 256, F16) == 100 * 256 * 4
    assert _whiten(R=0) == 0                            # R = 0 does nothing (no HIP call)
    assert _moments(R=0, rows=None, acc=1, ws=None) == 0    # R = 0 with accumulate changes nothing (no HIP call)


def test_exports_and_cpu_tensors_are_rejected():
    assert M.Whitening is Whitening and "Whitening" in M.__all__ and "embedding_moments" in M.__all__
    with pytest.raises(MI355Error, match="GPU"):
        M.embedding_moments(torch.randn(4, 8))
    with pytest.raises(MI355Error, match="GPU"):
        Whitening.fit(torch.randn(4, 8))
    x, _ = whiten_ref.spectrum_rows(5, 50, 3, normalized=False)
    w = Whitening.from_moments(*whiten_ref.moments(x))
    with pytest.raises(MI355Error, match="GPU"):
        w.transform(torch.from_numpy(x))
    with pytest.raises(MI355Error):
        M.Gallery(7, "cpu").whitened(w)                 # 7 columns against a 5-column fit


def _fixture(D):
    x, _ = whiten_ref.spectrum_rows(D, 500, 7, normalized=False)
    n, s, o = whiten_ref.moments(x)
    lam = np.linalg.eigvalsh(whiten_ref.covariance(n, s, o)[1])
    assert D == 1 or whiten_ref.min_relative_gap(lam) >= 1e-3    # certified by the generator
    return x, n, s, o


def _close_rows(got, want):
    """Within 1e-6 of the row's largest entry (bias: one row)."""
    got, want = np.atleast_2d(got.astype(np.float64)), np.atleast_2d(want)
    tol = 1e-6 * np.abs(want).max(1, keepdims=True)
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / np.abs(want).max(1, keepdims=True)).max())


@pytest.mark.parametrize("power", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("D", [1, 5, 64])
def test_from_moments_matches_the_float64_reference(D, power):
    x, n, s, o = _fixture(D)
    for d in sorted({1, max(D // 2, 1), D}):
        w = Whitening.from_moments(n, torch.from_numpy(s), torch.from_numpy(o), d, power=power)
        ref = whiten_ref.from_moments(n, s, o, d, power=power)
        assert (w.dim_in, w.dim_out, w.num_rows, w.power, w.ridge, w.normalize_input) == (D, d, n, power, 1e-5, True)
        assert w.matrix.dtype == torch.float32 and tuple(w.matrix.shape) == (d, D) and tuple(w.bias.shape) == (d,)
        _close_rows(w.matrix.numpy(), ref["matrix"])
        _close_rows(w.bias.numpy(), ref["bias"])
        np.testing.assert_allclose(w.mean.numpy(), ref["mean"], rtol=1e-6, atol=1e-7)
        lam = w.eigenvalues.numpy()
        assert w.eigenvalues.dtype == torch.float64 and lam.shape == (D,)
        assert (np.diff(lam) <= 0).all() and (lam >= 0).all()                       # descending, clamped
        np.testing.assert_allclose(lam, ref["eigenvalues"], rtol=1e-9, atol=1e-12 * lam[0])
        np.testing.assert_allclose(w.explained_variance_ratio.numpy(), ref["explained_variance_ratio"], rtol=1e-9, atol=1e-12)
        # sign rule: in each row of matrix (a positive multiple of an eigenvector) the first largest magnitude is positive
        m64 = ref["matrix"]
        top = np.abs(m64).argmax(1)
        assert (w.matrix.numpy()[np.arange(d), top] > 0).all()


@pytest.mark.parametrize("D", [5, 64])
def test_whitening_makes_the_covariance_the_identity(D):
    x, n, s, o = _fixture(D)
    w = Whitening.from_moments(n, s, o, power=0.5, ridge=0.0)                       # numpy float64 moments are accepted
    C = whiten_ref.covariance(n, s, o)[1]
    m = w.matrix.numpy().astype(np.float64)
    assert np.abs(m @ C @ m.T - np.eye(D)).max() <= 1e-5
    # and the bias centres: matrix mu + bias = 0 up to the fp32 rounding of both
    mu = s / n
    assert np.abs(m @ mu + w.bias.numpy()).max() <= 1e-5 * np.abs(m @ mu).max()


def test_from_moments_errors():
    x, n, s, o = _fixture(5)
    good = dict(n=n, sum=s, outer=o)

    def bad(**kw):
        args = {**good, **kw}
        with pytest.raises(MI355Error):
            Whitening.from_moments(args.pop("n"), args.pop("sum"), args.pop("outer"), **args)

    bad(n=1)
    bad(n=0)
    bad(n=2.5)
    bad(dim_out=0)
    bad(dim_out=6)
    bad(dim_out=2.0)
    bad(power=-0.1)
    bad(power=float("nan"))
    bad(ridge=-1e-3)
    bad(sum=s[:4])
    bad(outer=o[:, :4])
    bad(sum=s.astype(np.float32))
    bad(outer=torch.from_numpy(o).float())
    bad(sum=[0.0] * 5)
    s_nan = s.copy()
    s_nan[2] = np.nan
    bad(sum=s_nan)
    o_inf = o.copy()
    o_inf[1, 1] = np.inf
    bad(outer=o_inf)
    # zero eigenvalues among the kept ones: identical rows (0.5 everywhere: the covariance is exactly zero)
    nz, sz, oz = whiten_ref.moments(np.full((4, 5), 0.5))
    with pytest.raises(MI355Error):
        Whitening.from_moments(nz, sz, oz, power=0.5, ridge=0.0)
    with pytest.raises(MI355Error):
        Whitening.from_moments(nz, sz, oz, power=0.5, ridge=1e-5)                    # ridge * lambda_0 = 0 lifts nothing
    Whitening.from_moments(nz, sz, oz, power=0.0, ridge=0.0)                         # power 0 never divides
    # rows confined to a plane of R^5: the two kept eigenvalues are positive
    rng = np.random.default_rng(0)
    flat = rng.standard_normal((40, 2)) @ rng.standard_normal((2, 5))
    Whitening.from_moments(*whiten_ref.moments(flat), 2, power=0.5, ridge=0.0)


def test_state_dict_round_trip_gives_equal_bits():
    x, n, s, o = _fixture(64)
    w = Whitening.from_moments(n, s, o, 16, power=0.25, ridge=1e-4, normalize_input=False)
    sd = w.state_dict()
    w2 = Whitening().load_state_dict(sd)
    for k in ("mean", "matrix", "bias", "eigenvalues", "explained_variance_ratio"):
        a, b = getattr(w, k), getattr(w2, k)
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a.numpy().view(np.uint8), b.numpy().view(np.uint8)), k
    for k in ("dim_in", "dim_out", "num_rows", "power", "ridge", "normalize_input"):
        assert getattr(w, k) == getattr(w2, k), k
    sd["matrix"][0, 0] += 1.0                                                       # the state is a copy
    assert w.matrix[0, 0] != sd["matrix"][0, 0]
    with pytest.raises(MI355Error):
        Whitening().load_state_dict({k: v for k, v in sd.items() if k != "bias"})
    assert w.to("cpu") is w


def test_the_reference_whitens_a_hand_worked_example():
    # rows (+-2, 0) and (0, +-1): mean 0, covariance diag(2, 0.5); whitening scales the axes by 1/sqrt(2) and sqrt(2)
    x = np.array([[2.0, 0.0], [-2.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    ref = whiten_ref.from_moments(*whiten_ref.moments(x), ridge=0.0)
    np.testing.assert_allclose(ref["eigenvalues"], [2.0, 0.5], atol=1e-15)
    np.testing.assert_allclose(ref["matrix"], [[2 ** -0.5, 0.0], [0.0, 2 ** 0.5]], atol=1e-15)
    np.testing.assert_allclose(ref["bias"], [0.0, 0.0], atol=1e-15)
    y = whiten_ref.transform(x, ref["matrix"], ref["bias"], normalize_input=False, normalize_output=False)
    np.testing.assert_allclose(y, x * [2 ** -0.5, 2 ** 0.5], atol=1e-15)
    # PCA truncation (power 0, d = 1) keeps the x axis
    ref0 = whiten_ref.from_moments(*whiten_ref.moments(x), dim_out=1, power=0.0)
    np.testing.assert_allclose(ref0["matrix"], [[1.0, 0.0]], atol=1e-15)
