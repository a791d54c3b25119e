"""The NumPy model of the int8 gallery (gallery_i8_ref.py) alone, against float64 cosines qn . n: the per-pair error bound that
follows from the two quantisations, recall@10 against the exact top-10, and the range of the query's lo plane.  No GPU."""
import numpy as np
import pytest

import gallery_i8_ref as R

F32 = np.float32


def _normalize(x):
    x = x.astype(F32)
    return (x / np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)), 1e-6)[:, None].astype(F32)).astype(F32)


def _rows(kind, n, D, rng, centres):
    if kind == "normal":
        return rng.standard_normal((n, D))
    return centres[rng.integers(0, centres.shape[0], n)] + rng.standard_normal((n, D))     # 100 clusters, unit noise


CASES = [(D, kind) for D in (70, 128, 1536) for kind in ("normal", "clusters")]
_cache = {}


def _case(D, kind):
    if (D, kind) not in _cache:
        G, Q = (5000, 64) if D == 70 else (20000, 256)
        rng = np.random.default_rng(1000 + D + (7 if kind == "clusters" else 0))
        centres = rng.standard_normal((100, D))
        n, qn = _normalize(_rows(kind, G, D, rng, centres)), _normalize(_rows(kind, Q, D, rng, centres))
        codes, s_g = R.quantize_rows(n)
        hi, lo, s_q = R.query_planes(qn)
        s = R.scores(hi, lo, s_q, codes, s_g)
        exact = qn.astype(np.float64) @ n.astype(np.float64).T
        _cache[(D, kind)] = dict(n=n, qn=qn, codes=codes, s_g=s_g, hi=hi, lo=lo, s_q=s_q, s=s, exact=exact)
    return _cache[(D, kind)]


@pytest.mark.parametrize("D,kind", CASES)
def test_error_bound_of_every_pair(D, kind):
    c = _case(D, kind)
    deq_l1 = (np.abs(c["codes"].astype(np.float64)).sum(axis=1) * c["s_g"].astype(np.float64))          # |g^|_1
    q_l1 = np.abs(c["qn"].astype(np.float64)).sum(axis=1)
    bound = (c["s_g"].astype(np.float64) / 2)[None, :] * q_l1[:, None] + (c["s_q"].astype(np.float64) / 256)[:, None] * deq_l1[None, :] + 1e-6
    err = np.abs(c["s"].astype(np.float64) - c["exact"])
    print(f"D={D} {kind}: max err {err.max():.3e} rms {np.sqrt((err ** 2).mean()):.3e} least slack {(bound - err).min():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("D,kind", CASES)
def test_recall_at_10(D, kind):
    c = _case(D, kind)
    got = R.topk(c["s"], 10)[1]
    want = np.argsort(-c["exact"], axis=1, kind="stable")[:, :10]
    recall = (got[:, :, None] == want[:, None, :]).any(axis=1).mean()
    print(f"D={D} {kind}: recall@10 {recall:.4f}")
    assert recall >= 0.95


@pytest.mark.parametrize("D,kind", CASES)
def test_plane_ranges(D, kind):
    c = _case(D, kind)
    assert np.abs(c["lo"].astype(np.int32)).max() <= 64
    assert np.abs(c["hi"].astype(np.int32)).max() == 127 and np.abs(c["codes"].astype(np.int32)).max() == 127
    acc_hi = np.abs(c["hi"].astype(np.float64) @ c["codes"].astype(np.float64).T).max()
    assert acc_hi < 2 ** 24                                          # float(acc_hi) is exact at these widths


def test_exact_ties_go_to_the_even_code():
    """The model against the codes written out by hand: half to even, never half away from zero or half up."""
    assert R.TIES.tolist() == [0.5, 1.5, 2.5, 3.5, 125.5, 126.5, -0.5, -1.5, -2.5, -3.5, -125.5, -126.5, 127, -127, 126.75, 0.25, -0.25]
    assert R.TIE_CODES.tolist() == [0, 2, 2, 4, 126, 126, 0, -2, -2, -4, -126, -126, 127, -127, 127, 0, 0]
    away = np.sign(R.TIES) * np.floor(np.abs(R.TIES) + F32(0.5))     # half away from zero, and half up: both miss ties
    assert (away.astype(np.int8) != R.TIE_CODES).sum() == 6 and (np.floor(R.TIES + F32(0.5)).astype(np.int8) != R.TIE_CODES).sum() == 6
    for D in (17, 68, 70):
        rows, want, scales = R.tie_rows(D)
        assert rows.dtype == F32 and (np.abs(rows).max(axis=1) == F32(127) * scales).all()
        assert (rows[1] * F32(8) == rows[0]).all() and (rows[2] == rows[0] * F32(64)).all()         # the scalings are exact
        codes, s = R.quantize_rows(rows)
        assert (codes == want[None, :]).all() and (want[:17] == R.TIE_CODES).all()
        assert (s.view(np.int32) == scales.view(np.int32)).all() and scales.tolist() == [1.0, 0.125, 64.0]
        assert (codes.view(np.uint8)[:, 6] == 0).all()               # -0.5 -> the byte 0x00
    n = np.full((2, 8), 0.25, F32)
    n[0, 5] = np.inf                                                 # a non-finite amax without a NaN element
    n[1] = F32(1e-31) * np.array([1, -1, 0.5, 0, 1, 0.25, -0.5, 1], F32)   # a non-zero row below 1e-30
    codes, s = R.quantize_rows(n)
    assert not np.isnan(n).any() and (codes == 0).all() and np.isnan(s[0]) and s[1] == 0 and np.abs(n[1]).max() == F32(1e-31)


def test_special_rows():
    n = np.zeros((5, 8), F32)
    n[1, 3] = np.nan
    n[2, 2] = -0.5
    n[3] = 0.25
    n[4] = 1e-31
    codes, s = R.quantize_rows(n)
    assert (codes[0] == 0).all() and s[0] == 0
    assert (codes[1] == 0).all() and np.isnan(s[1])
    assert codes[2].tolist() == [0, 0, -127, 0, 0, 0, 0, 0] and s[2] == F32(0.5) / F32(127)
    assert (codes[3] == 127).all()
    assert (codes[4] == 0).all() and s[4] == 0
    hi, lo, s_q = R.query_planes(n)
    assert (lo[0] == 0).all() and (lo[1] == 0).all() and (lo[4] == 0).all()
    sc = R.scores(hi, lo, s_q, codes, s)
    assert np.isnan(sc[1]).all() and np.isnan(sc[:, 1]).all()        # a NaN query / row scores NaN everywhere
    assert (sc[[0, 2, 3, 4]][:, [0, 4]] == 0).all()                  # a zero row scores 0
    v, i = R.topk(sc[2:4], 3)
    assert i[:, 0].tolist() == [1, 1] and np.isnan(v[:, 0]).all()    # NaN first
    v, i = R.topk(sc[2:4], 3, mask=np.array([[0, 0, 1, 1, 0], [0, 0, 0, 0, 0]], bool))
    assert i.tolist() == [[2, 3, -1], [-1, -1, -1]] and v[1].tolist() == [-np.inf] * 3 and v[0, 2] == -np.inf
