"""The NumPy model of the score normalisation (tests/scorenorm_ref.py) on its own, without a GPU: the planted-hub fixture does
what it is for, and the model has the properties the definitions promise."""
import numpy as np

import scorenorm_ref as SR

F32 = np.float32


def _slabs(seed=0):
    f = SR.hub_fixture(seed)
    return f, SR.cosine(f["gallery"], f["cohort"]), SR.cosine(f["queries"], f["gallery"]), SR.cosine(f["queries"], f["cohort"])


def test_csls_removes_the_planted_hubs():
    f, Sgc, Sqg, Sqc = _slabs(0)
    plain = SR.topk(Sqg, 1)[1]
    aq, bq, ag, bg = SR.coefficients("csls", Sgc, Sqg, Sqc)
    csls = SR.topk(SR.adjust(Sqg, aq, bq, ag, bg), 1)[1]
    p_plain = SR.precision_at_1(plain, f["query_labels"], f["gallery_labels"])
    p_csls = SR.precision_at_1(csls, f["query_labels"], f["gallery_labels"])
    hubs = float((f["gallery_labels"][plain[:, 0]] == -1).mean())
    print(f"precision@1 plain {p_plain:.3f}, CSLS {p_csls:.3f}; hub rows among the plain top-1: {hubs:.2f}")
    assert p_plain < 0.6 and p_csls > 0.9
    assert hubs > 0.4


def test_the_csls_order_of_a_query_does_not_depend_on_bq():
    f, Sgc, Sqg, Sqc = _slabs(1)
    aq, bq, ag, bg = SR.coefficients("csls", Sgc, Sqg, Sqc)
    # exact arithmetic: a per-query constant moves a whole row of t.  In fp32 the subtraction rounds, so the check is on
    # coefficients whose sums are exact: multiples of 2^-6 next to scores rounded to multiples of 2^-12
    S = np.round(Sqg * 4096) / 4096
    bgq = (np.round(bg * 64) / 64).astype(F32)
    a = SR.topk(SR.adjust(S.astype(F32), aq, (np.round(bq * 64) / 64).astype(F32), None, bgq), 10)[1]
    b = SR.topk(SR.adjust(S.astype(F32), aq, np.zeros_like(bq), None, bgq), 10)[1]
    assert np.array_equal(a, b)


def test_znorm_with_the_whole_cohort_standardises_every_gallery_column():
    f, Sgc, Sqg, Sqc = _slabs(2)
    aq, bq, ag, bg = SR.coefficients("znorm", Sgc, Sqg, Sqc)
    assert aq is None and bq is None
    Z = SR.adjust(SR.cosine(f["cohort"], f["gallery"]), None, None, ag, bg).astype(np.float64)
    assert np.abs(Z.mean(0)).max() < 1e-4 and np.abs(Z.std(0) - 1).max() < 1e-4


def test_snorm_is_the_mean_of_znorm_and_tnorm():
    """Within 2 fp32 ulp, the ulp taken where the roundings happen: at U = spacing(Mz + Mt), Mz = max(|s ag|, |bg|) and Mt =
    max(|s aq|, |bq|) the operands of the z and the t slab (the result itself is their small difference: near a score equal to
    the cohort mean it cancels to 0, where an ulp of the result means nothing - 12288 of them were measured on this fixture).
    Why 2 U: z rounds its product and its difference, each by at most spacing(Mz) / 2 <= U / 2, t likewise, so their mean is off
    by at most U; s works at half that magnitude, spacing U / 2, and rounds four times (aq + ag, the product, bq + bg, the
    difference): at most U again.  The halved coefficients themselves are exact halves.  Measured: at most 1.875 U over seeds
    0 to 7 and n = None, 30, 5."""
    f, Sgc, Sqg, Sqc = _slabs(3)
    for n in (None, 30):
        cz, ct = SR.coefficients("znorm", Sgc, Sqg, Sqc, n), SR.coefficients("tnorm", Sgc, Sqg, Sqc, n)
        z, t = SR.adjust(Sqg, *cz), SR.adjust(Sqg, *ct)
        s = SR.adjust(Sqg, *SR.coefficients("snorm", Sgc, Sqg, Sqc, n))
        want = (z.astype(np.float64) + t.astype(np.float64)) / 2
        Mz = np.maximum(np.abs(Sqg * cz[2][None, :]), np.abs(cz[3])[None, :])
        Mt = np.maximum(np.abs(Sqg * ct[0][:, None]), np.abs(ct[1])[:, None])
        U = np.spacing((Mz + Mt).astype(F32)).astype(np.float64)
        worst = float((np.abs(s - want) / U).max())
        print(f"n={n}: snorm against the mean of znorm and tnorm: at most {worst:.3f} ulp")
        assert worst <= 2.0


def test_the_adaptive_variant_uses_the_top_n_only():
    f, Sgc, Sqg, Sqc = _slabs(4)
    whole = SR.coefficients("snorm", Sgc, Sqg, Sqc)
    top = SR.coefficients("snorm", Sgc, Sqg, Sqc, n=30)
    assert all(w.shape == t.shape and not np.array_equal(w, t) for w, t in zip(whole, top))
    vals, idx = SR.topk(Sgc, 30)
    mean = vals.astype(np.float64).mean(1)
    assert np.allclose(top[3], 0.5 * mean / np.maximum(vals.astype(np.float64).std(1), 1e-6), rtol=1e-5)


def test_topk_orders_like_the_library():
    T = np.array([[1.0, np.nan, 1.0, -np.inf, 0.0, -0.0]], F32)
    v, i = SR.topk(T, 6, off=10)
    assert i.tolist() == [[11, 10, 12, 14, 15, 13]] and np.isnan(v[0, 0]) and v[0, 5] == -np.inf
    v, i = SR.topk(T, 4, elig=np.array([[True, False, True, False, False, True]]))
    assert i.tolist() == [[0, 2, 5, -1]] and v[0, 3] == -np.inf


def test_stats_of_pads_and_empty_rows():
    vals = np.array([[0.5, 0.25, -np.inf], [-np.inf] * 3, [0.125] * 3], F32)
    idx = np.array([[4, 9, -1], [-1, -1, -1], [0, 1, 2]], np.int64)
    mean, std, cnt, a, b = SR.topn_stats(vals, idx, 0.5, 1e-6)
    assert cnt.tolist() == [2, 0, 3] and mean.tolist() == [0.375, 0.0, 0.125] and std.tolist() == [0.125, 0.0, 0.0]
    assert a.tolist() == [4.0, F32(0.5 / 1e-6), F32(0.5 / 1e-6)] and b[0] == 1.5 and b[1] == 0.0
