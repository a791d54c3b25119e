"""The NumPy model of the fp4 gallery (gallery_fp4_ref.py) against a float64 restatement of the contract, and the properties the
format rests on: the residual of the hi plane stays within one step, every dot product is exact in fp32, the packing, and the
recall the GPU test then only has to reproduce.  No GPU."""
import numpy as np
import pytest

import gallery_fp4_ref as R

F32 = np.float32
MAGS64 = R.MAGNITUDES.astype(np.float64)


def _e2m1_f64(a):
    """The nearest magnitude by distance in float64, a tie to the even index; sign in bit 3, no negative zero."""
    a = np.asarray(a, dtype=np.float64)
    d = np.abs(np.abs(a)[..., None] - MAGS64)
    best = d.min(axis=-1, keepdims=True)
    tied = d == best
    even = tied & (np.arange(8) % 2 == 0)
    idx = np.where(tied.sum(axis=-1) > 1, even.argmax(axis=-1), tied.argmax(axis=-1))
    return (idx | np.where((a < 0) & (idx > 0), 8, 0)).astype(np.uint8)


def _unit(x):
    x = np.asarray(x, dtype=np.float64)
    return (x / np.sqrt((x * x).sum(axis=1))[:, None]).astype(F32)


def _tie_values():
    """Every tie threshold, its two float32 neighbours, the magnitudes themselves, 6 and beyond, both signs."""
    t = np.concatenate([R.TIES, np.nextafter(R.TIES, F32(0)), np.nextafter(R.TIES, F32(10)), R.MAGNITUDES,
                        np.array([5.999, 6.0, 6.5, 100.0, 1e-30, 0.2499], F32)]).astype(F32)
    return np.concatenate([t, -t])


def test_e2m1_rounds_to_nearest_ties_to_even():
    v = _tie_values()
    assert (R.e2m1(v) == _e2m1_f64(v)).all()
    want = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0, 6.0: 6.0, 7.0: 6.0, 1e9: 6.0}
    for a, m in want.items():
        assert R.value(R.e2m1(F32(a))) == F32(m) and R.value(R.e2m1(F32(-a))) == F32(-m), a
    assert R.e2m1(F32(-0.1)) == 0 and R.e2m1(F32(-0.0)) == 0         # no negative zero
    a = (np.random.default_rng(1).standard_normal(100000) * 3).astype(F32)
    assert (R.e2m1(a) == _e2m1_f64(a)).all()
    assert (R.value(np.arange(16)) == np.concatenate([R.MAGNITUDES, -R.MAGNITUDES])).all()
    assert (R.twice(np.arange(16)) == 2 * R.value(np.arange(16))).all()


@pytest.mark.parametrize("D", [1, 2, 255, 256, 257, 1536])
def test_row_quantiser_against_float64(D):
    rng = np.random.default_rng(D)
    n = _unit(rng.standard_normal((300, D)))
    n[3] = 0
    n[10, D // 2] = np.nan
    n[20] = 0
    n[20, D - 1] = -1.0
    codes, mult = R.quantize_rows(n)
    assert codes.shape == (300, D) and codes.dtype == np.uint8 and mult.dtype == F32
    assert (codes[3] == 0).all() and mult[3] == 0 and (codes[10] == 0).all() and np.isnan(mult[10])
    assert codes[20, D - 1] == 8 | 7 and mult[20] == F32(1 / 6)
    live = np.isfinite(mult) & (mult != 0)
    a = n[live].astype(np.float64) * (6.0 / np.abs(n[live]).max(axis=1).astype(np.float64))[:, None]
    near_tie = (np.abs(np.abs(a)[..., None] - R.TIES.astype(np.float64)) < 1e-5).any(axis=-1)
    assert ((codes[live] == _e2m1_f64(a)) | near_tie).all()           # fp32 rounding of a may cross a threshold only there
    assert (np.abs(R.twice(codes[live])).max(axis=1) == 12).all()     # the largest element is +-6
    norm = np.sqrt((R.value(codes[live]).astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(mult[live] * norm - 1).max() < 3e-7                 # mult = 1 / |value(codes)|, two fp32 roundings
    deq = R.value(codes[live]) * mult[live, None]
    cos = (deq.astype(np.float64) * n[live]).sum(axis=1)
    assert cos.min() > (0.95 if D > 2 else 0.7), cos.min()            # the decoded row points where the row points


def test_residual_stays_within_one_step():
    rng = np.random.default_rng(7)
    qn = _unit(rng.standard_normal((500, 256)))
    ties = _tie_values()
    ties = ties[np.abs(ties) <= 6]
    # amax = 6 * 2^e: 6 / amax and amax / 6 are exact, the values sit exactly on the thresholds and |r| <= 1 holds as it stands.
    # Any other amax puts them within a rounding of a threshold, and r within two roundings of +-1: the plane still holds it
    exact, near = (1.0, 0.125, 2.0 ** -10), (1 / 3, 0.01, 0.37, 1e-3)
    rows = [np.concatenate([ties, [6.0]]).astype(F32) * F32(s) for s in exact + near]
    for q, bound in ((qn, 1.0), (np.stack(rows[:3]), 1.0), (np.stack(rows[3:]), 1.0 + 2.0 ** -22)):
        hi, lo, s_q = R.query_planes(q)
        r = R.residuals(q, hi, s_q)
        assert np.abs(r).max() <= bound, np.abs(r).max()
        assert np.abs(R.twice(lo)).max() <= 8 and np.abs(R.twice(hi)).max() == 12
    hi, lo, s_q = R.query_planes(np.stack(rows)[:1])                  # amax = 6: s_q = 1, the planes of the values themselves
    assert s_q[0] == 1 and (hi[0] == R.e2m1(rows[0])).all()
    back = R.value(hi[0]).astype(np.float64) + R.value(lo[0]).astype(np.float64) / 4
    assert np.abs(back - rows[0]).max() <= 0.125                      # lo steps by 0.5 / 4 or 1 / 4: half a step of error at most
    z = np.zeros((3, 8), F32)
    z[1, 2] = np.nan
    z[2, 0] = 1e-35
    hi, lo, s_q = R.query_planes(z)
    assert (hi == 0).all() and (lo == 0).all() and s_q[0] == 0 and np.isnan(s_q[1]) and s_q[2] == 0


def test_sums_are_exact_in_fp32_up_to_the_dimension_cap():
    assert 36 * 65536 * 4 < 2 ** 24
    assert int(np.abs(R.twice(np.arange(16))).max()) ** 2 == 36 * 4   # the largest product, in quarters
    D = 65536
    c = np.full((2, D), 7, np.uint8)                                  # +6 everywhere
    c[1, -100:] = 8 | 1                                               # ... but a trailing run of -0.5
    s = R.scores(c, c, np.ones(2, F32), c, np.ones(2, F32))           # asserts that acc_hi and acc_lo are float32 values
    assert s[0, 0] == F32(36 * D * 1.25) and s[1, 1] == F32((36 * (D - 100) + 25) * 1.25)
    assert s[0, 1] == F32((36 * (D - 100) - 300) * 1.25)


@pytest.mark.parametrize("D", [1, 2, 255, 256, 257, 600])
def test_packing_and_padding(D):
    rng = np.random.default_rng(D)
    codes = rng.integers(0, 16, (5, D)).astype(np.uint8)
    p = R.pack(codes)
    ld = R.stride(D)
    assert p.shape == (5, ld) and ld % 128 == 0 and ld >= (D + 1) // 2 and ld - (D + 1) // 2 < 128
    assert (p[:, : D // 2] & 15 == codes[:, 0: D - D % 2: 2]).all() and (p[:, : D // 2] >> 4 == codes[:, 1::2]).all()
    if D % 2:
        assert (p[:, D // 2] == codes[:, -1]).all()                   # the last low nibble, a zero high nibble
    assert (p[:, (D + 1) // 2:] == 0).all()
    assert (R.unpack(p, D) == codes).all()
    assert [R.stride(d) for d in (1, 256, 257, 1536, 65536)] == [128, 128, 256, 768, 32768]


def test_scores_against_float64():
    rng = np.random.default_rng(11)
    n, qn = _unit(rng.standard_normal((400, 200))), _unit(rng.standard_normal((30, 200)))
    n[5] = 0
    n[6, 3] = np.nan
    qn[2] = 0
    qn[3, 1] = np.nan
    codes, mult = R.quantize_rows(n)
    hi, lo, s_q = R.query_planes(qn)
    s = R.scores(hi, lo, s_q, codes, mult)
    assert s.dtype == F32 and s.shape == (30, 400)
    assert np.isnan(s[3]).all() and np.isnan(s[:, 6]).all() and (s[2, np.arange(400) != 6] == 0).all()
    assert (s[np.arange(30) != 3, 5] == 0).all()
    ok_q, ok_g = np.isfinite(s_q) & (s_q != 0), np.isfinite(mult) & (mult != 0)
    qd = (R.value(hi).astype(np.float64) + R.value(lo).astype(np.float64) / 4) * s_q.astype(np.float64)[:, None]
    gd = R.value(codes).astype(np.float64) * mult.astype(np.float64)[:, None]
    want = qd[ok_q] @ gd[ok_g].T
    assert np.abs(s[ok_q][:, ok_g] - want).max() < 3e-7               # three fp32 roundings of a value below 1
    assert np.abs(qd[ok_q] - qn[ok_q]).max() <= np.abs(qn[ok_q]).max() / 6 * 0.125 * 1.001   # the query keeps two planes
    exact = qn[ok_q].astype(np.float64) @ n[ok_g].astype(np.float64).T
    assert np.abs(s[ok_q][:, ok_g] - exact).max() < 0.1               # four bits: a few per cent of a unit cosine


def test_recall_on_a_planted_mixture():
    """The bounds of the GPU test (tests/test_gallery_fp4_gpu.py), which asserts that the library returns the model's lists."""
    m = R.mixture_model()
    print(f"fp4 model on the planted mixture: raw recall@10 {m['raw']:.4f}, refined at a shortlist of 30 {m['refined']:.4f}")
    assert m["raw"] >= 0.85
    assert m["refined"] == 1.0
