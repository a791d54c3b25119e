"""PCA whitening on the MI355X against the float64 reference of tests/whiten_ref.py: the f64-MFMA moments
(mi355_embedding_moments), the fused transform (mi355_whiten_rows), the fit, Gallery.whitened and the end-to-end retrieval
gain.  Every bound is derived (summation / dot-product rounding bounds of the number formats), none is measured."""
import numpy as np
import pytest
import torch

import whiten_ref
import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import Whitening, embedding_moments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows(R, D, seed):
    """fp32 rows with a common offset (co-linear, as GAP embeddings are) and mixed signs."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((R, D)) + 0.75).astype(np.float32)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _check_moments(m, x64, what):
    """|err[i][j]| <= 2 R 2^-53 sum_r |x_ri x_rj| (f64 summation of exact products, factor 2 for the reference's own sum);
    the same bound with |x_ri| for the row sums; outer exactly symmetric."""
    R = x64.shape[0]
    n, s, o = whiten_ref.moments(x64)
    assert m.n == n, what
    go, gs = m.outer.cpu().numpy(), m.sum.cpu().numpy()
    bound_o = 2.0 * R * 2.0 ** -53 * whiten_ref.abs_outer(x64)
    bound_s = 2.0 * R * 2.0 ** -53 * np.abs(x64).sum(0)
    eo, es = np.abs(go - o), np.abs(gs - s)
    print(f"{what}: outer err / bound max {np.max(eo / np.maximum(bound_o, 1e-300)):.3g}, sum {np.max(es / np.maximum(bound_s, 1e-300)):.3g}")
    assert (eo <= bound_o).all(), what
    assert (es <= bound_s).all(), what
    assert np.array_equal(go, go.T), what


@pytest.mark.parametrize("D", [1, 7, 64, 70, 1536])
@pytest.mark.parametrize("R", [1, 37, 1000, 4099])
def test_moments_against_float64(R, D):
    xn = _rows(R, D, 100 * D + R)
    x = torch.from_numpy(xn).to(DEV)
    # fp32 rows, contiguous
    m = embedding_moments(x)
    _check_moments(m, xn.astype(np.float64), "contiguous")
    m2 = embedding_moments(x)
    assert np.array_equal(_bits(m.outer), _bits(m2.outer)) and np.array_equal(_bits(m.sum), _bits(m2.sum))   # same call, same bits
    # ld > dim: the rows as columns [3, 3 + D) of a wider buffer
    wide = torch.full((R, D + 9), 7.0, dtype=torch.float32, device=DEV)
    wide[:, 3: 3 + D] = x
    _check_moments(embedding_moments(wide[:, 3: 3 + D]), xn.astype(np.float64), "strided")
    # normalised on the fly: the reference is fed the library's own normalised rows, so only the summation differs
    xl = M.l2_normalize_rows(x).cpu().numpy().astype(np.float64)
    _check_moments(embedding_moments(x, normalize=True), xl, "normalize")
    # fp16 gallery rows, widened exactly
    g = M.Gallery(D, DEV, dtype=torch.float16).add(x)
    mh = g.moments()
    _check_moments(mh, g.data.cpu().numpy().astype(np.float64), "fp16 gallery")
    # two accumulate calls over a split of the rows: the same bound, and the same bits when the sequence is repeated
    if R >= 2:
        h = R // 3 + 1

        def two_calls():
            a = embedding_moments(x[:h])
            return embedding_moments(x[h:], out=a)

        t1, t2 = two_calls(), two_calls()
        _check_moments(t1, xn.astype(np.float64), "accumulate")
        assert np.array_equal(_bits(t1.outer), _bits(t2.outer)) and np.array_equal(_bits(t1.sum), _bits(t2.sum))


def test_moments_of_no_rows_and_nan_rows():
    D = 70
    x = torch.from_numpy(_rows(50, D, 5)).to(DEV)
    m = embedding_moments(x)
    keep_o, keep_s = m.outer.clone(), m.sum.clone()
    m0 = embedding_moments(x[:0], out=m)                                  # R = 0 with accumulate changes nothing
    assert m0.n == 50 and torch.equal(m0.outer, keep_o) and torch.equal(m0.sum, keep_s)
    z = embedding_moments(x[:0])                                          # without: zeros
    assert z.n == 0 and not z.outer.any() and not z.sum.any()
    xb = x.clone()
    xb[7, 3] = float("nan")
    mb = embedding_moments(xb)
    assert torch.isnan(mb.outer[3]).all() and torch.isnan(mb.outer[:, 3]).all() and torch.isnan(mb.sum[3])
    rest = torch.ones(D, dtype=torch.bool)
    rest[3] = False
    assert torch.isfinite(mb.outer[rest][:, rest]).all()


def _make(D, d, seed, normalize_input=True):
    """A Whitening with a random projection (the transform kernel does not care where matrix and bias come from)."""
    rng = np.random.default_rng(seed)
    w = Whitening()
    w.dim_in, w.dim_out, w.num_rows, w.normalize_input = D, d, 1000, normalize_input
    w.matrix = torch.from_numpy((rng.standard_normal((d, D)) * 3.0).astype(np.float32)).to(DEV)
    w.bias = torch.from_numpy((rng.standard_normal(d) * 0.1).astype(np.float32)).to(DEV)
    w.mean = torch.zeros(D, device=DEV)
    w.eigenvalues = torch.ones(D, dtype=torch.float64)
    w.explained_variance_ratio = torch.ones(d, dtype=torch.float64) / D
    return w


SHAPES = [(7, 3), (70, 70), (1536, 256), (1536, 1536), (2560, 128)]


@pytest.mark.parametrize("D, d", SHAPES)
def test_transform_against_float64(D, d):
    w = _make(D, d, D + d)
    R = 300
    x = torch.from_numpy(_rows(R, D, D * 3 + d)).to(DEV)
    y = w.transform(x, normalize_output=False)
    xp = M.l2_normalize_rows(x).cpu().numpy().astype(np.float64)         # the library's own normalised input
    m64, b64 = w.matrix.cpu().numpy().astype(np.float64), w.bias.cpu().numpy().astype(np.float64)
    ref, scale = whiten_ref.project(xp, m64, b64, normalize_input=False)
    bound = (D + 8) * 2.0 ** -24 * scale
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    print(f"transform {D}->{d}: err / bound max {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    # the normalised output is l2_normalize_rows of the un-normalised one, bit for bit
    yn = w.transform(x)
    assert np.array_equal(_bits(yn), _bits(M.l2_normalize_rows(y)))
    # out= and rows of a wider buffer
    wide = torch.zeros((R, D + 4), dtype=torch.float32, device=DEV)
    wide[:, :D] = x
    out = torch.empty((R, d), dtype=torch.float32, device=DEV)
    assert w.transform(wide[:, :D], out=out) is out and np.array_equal(_bits(out), _bits(yn))
    # without input normalisation the rows go in as they are
    w.normalize_input = False
    y_raw = w.transform(x, normalize_output=False).cpu().numpy().astype(np.float64)
    ref_raw, scale_raw = whiten_ref.project(x.cpu().numpy(), m64, b64, normalize_input=False)
    assert (np.abs(y_raw - ref_raw) <= (D + 8) * 2.0 ** -24 * scale_raw).all()


@pytest.mark.parametrize("D, d", SHAPES)
def test_a_row_does_not_depend_on_its_batch(D, d):
    w = _make(D, d, 2 * D + d)
    x = torch.from_numpy(_rows(300, D, D + 7 * d)).to(DEV)
    for R in (1, 63, 64, 65, 300):
        for norm_out in (True, False):
            y = w.transform(x[:R], normalize_output=norm_out)
            for i in sorted({0, 31, 32, 62, 63, 64, 127, 128, 255, 256, R - 1}):
                if i < R:
                    one = w.transform(x[i: i + 1], normalize_output=norm_out)
                    assert np.array_equal(_bits(y[i]), _bits(one[0])), (R, i, norm_out)


@pytest.mark.parametrize("D, d", SHAPES)
def test_fp16_output_is_the_fp16_gallery_storage(D, d):
    w = _make(D, d, 3 * D + d, normalize_input=False)
    x = torch.from_numpy(_rows(130, D, 11 * D + d)).to(DEV)
    g = M.Gallery(D, DEV).add(x)
    y = w.transform(g.data, normalize_output=False)                       # the resident rows go in as they are
    want = M.Gallery(d, DEV, dtype=torch.float16).add(y)
    got = g.whitened(w, dtype=torch.float16)
    assert got.dtype == torch.float16 and got.rows == 130 and got.dim == d
    assert np.array_equal(_bits(got._buf[:130]), _bits(want._buf[:130]))  # pads included
    assert not got._buf[:130, d:].any()
    # an fp16 source gallery: its rows widened exactly
    gh = M.Gallery(D, DEV, dtype=torch.float16).add(x)
    yh = w.transform(gh.data.float(), normalize_output=False)
    assert np.array_equal(_bits(gh.whitened(w)._buf[:130]), _bits(M.Gallery(d, DEV, dtype=torch.float16).add(yh)._buf[:130]))
    assert np.array_equal(_bits(gh.whitened(w, dtype=torch.float32).data), _bits(M.l2_normalize_rows(yh)))


def _close_rows(got, want):
    """Within 1e-6 of the row's largest entry (bias: one row): float64 results rounded once to fp32."""
    got, want = np.atleast_2d(got.astype(np.float64)), np.atleast_2d(want)
    rel = np.abs(got - want) / np.abs(want).max(1, keepdims=True)
    print(f"fit: max deviation relative to the row's largest entry {rel.max():.3g}")
    assert (rel <= 1e-6).all()


@pytest.mark.parametrize("D", [64, 70])
def test_fit_against_float64(D):
    xn, _ = whiten_ref.spectrum_rows(D, 4000, 5)
    x = torch.from_numpy(xn).to(DEV)
    d = D // 2
    g32 = M.Gallery(D, DEV).add(x)
    g16 = M.Gallery(D, DEV, dtype=torch.float16).add(x)
    cases = [("tensor", lambda: Whitening.fit(x, d, block=1500), M.l2_normalize_rows(x)),
             ("gallery fp32", lambda: Whitening.fit(g32, d), g32.data),
             ("gallery fp16", lambda: Whitening.fit(g16, d), g16.data)]
    for what, fit, stored in cases:
        s64 = stored.cpu().numpy().astype(np.float64)
        n, s, o = whiten_ref.moments(s64)
        lam = np.linalg.eigvalsh(whiten_ref.covariance(n, s, o)[1])
        assert whiten_ref.min_relative_gap(lam) >= 1e-3, what            # the fixture's certificate holds for the stored rows
        ref = whiten_ref.from_moments(n, s, o, d)
        w = fit()
        assert (w.dim_in, w.dim_out, w.num_rows) == (D, d, 4000) and w.matrix.device.type == "cuda", what
        _close_rows(w.matrix.cpu().numpy(), ref["matrix"])
        _close_rows(w.bias.cpu().numpy(), ref["bias"])
        np.testing.assert_allclose(w.eigenvalues.numpy(), ref["eigenvalues"], rtol=1e-7, atol=1e-9 * ref["eigenvalues"][0])


def test_fit_at_1536_through_the_metric():
    """At D = 1536 neighbouring eigenvalues are too close to compare eigenvectors; matrix^T matrix = (C + ridge l0 I)^-1 does
    not depend on the choice of basis."""
    D, R = 1536, 4099
    x = torch.from_numpy(_rows(R, D, 1536)).to(DEV)
    w = Whitening.fit(x, block=2048)
    s64 = M.l2_normalize_rows(x).cpu().numpy().astype(np.float64)
    ref = whiten_ref.from_moments(*whiten_ref.moments(s64))
    m = w.matrix.cpu().numpy().astype(np.float64)
    got, want = m.T @ m, ref["matrix"].T @ ref["matrix"]
    dev = np.abs(got - want).max() / np.abs(want).max()
    print(f"metric at D=1536: max deviation {dev:.3g} of the largest entry")
    assert dev <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_whitened_gallery_search(dtype):
    D, d, k = 70, 24, 5
    xn, _ = whiten_ref.spectrum_rows(D, 1200, 9, normalized=False)
    raw = torch.from_numpy(xn[:1000].copy()).to(DEV)
    q = torch.from_numpy(xn[1000:].copy()).to(DEV)
    labels = torch.arange(1000, device=DEV) % 13
    g = M.Gallery(D, DEV, dtype=dtype).add(raw, labels)
    before = g._buf[:1000].clone()
    w = Whitening.fit(g, d)
    gw = g.whitened(w)
    assert torch.equal(g._buf[:1000], before) and gw.dim == d and gw.rows == 1000 and gw.dtype == dtype    # the source is not changed
    assert torch.equal(gw.labels, labels) and gw.labels is not g.labels
    tq = w.transform(q)
    v, i = gw.search(tq, k)
    if dtype == torch.float32:
        # the gallery's rows are w.transform of the raw rows: same normalisation bits, same projection
        assert np.array_equal(_bits(gw.data), _bits(w.transform(raw)))
        wv, wi = M.cosine_topk(tq, w.transform(raw), k, gallery_is_normalized=True)
    else:
        y = w.transform(g.data.float())                                   # (renormalising the stored fp16 rows is the only difference)
        wn = Whitening().load_state_dict(w.state_dict()).to(DEV)
        wn.normalize_input = False
        want = M.Gallery(d, DEV, dtype=torch.float16).add(wn.transform(g.data.float(), normalize_output=False))
        assert np.array_equal(_bits(gw._buf[:1000]), _bits(want._buf[:1000])) and y.shape == (1000, d)
        wv, wi = want.search(tq, k)
    assert torch.equal(i, wi) and np.array_equal(_bits(v), _bits(wv))
    # whiten, then query expansion / DBA on the whitened rows
    v2, i2 = gw.search(tq, k, qe=(4, 3.0))
    assert i2.shape == (200, k) and torch.isfinite(v2).all()


def test_end_to_end_whitening_recovers_the_classes():
    x_np, lab_np = whiten_ref.labelled_set(1)
    assert x_np.shape == (1000, 128)
    x, lab = torch.from_numpy(x_np).to(DEV), torch.from_numpy(lab_np).to(DEV)
    w = Whitening.fit(x, 32)
    acc = M.retrieval_accuracy(w.transform(x), lab, ks=(1,))
    raw = M.retrieval_accuracy(x, lab, ks=(1,))
    fit, y = whiten_ref.pipeline(x_np, 32)
    top1, gap, p_ref = whiten_ref.loo_top1(y, lab_np)
    certified = gap > 1e-4
    p_w, p_raw = float(acc["precision_at_1"].item()), float(raw["precision_at_1"].item())
    print(f"certified {certified.mean():.4f}, P@1 raw {p_raw:.3f}, whitened {p_w:.3f}, float64 reference {p_ref:.3f}")
    assert certified.mean() >= 0.95
    got = acc["indices"][:, 0].cpu().numpy()
    assert (got[certified] == top1[certified]).all()
    assert p_w - p_raw >= 0.5
