"""The NumPy model of result diversification (tests/diversify_ref.py) against a brute-force restatement and its own identities,
without a GPU, and the numbers of the ``products`` fixture on the model: what the GPU tests then ask of the library."""
import numpy as np
import pytest

import diversify_ref as dr
from imageretrievalresearch_amd import diversify  # noqa: F401  (the feature under test: these tests belong to it)

SEEDS = [0, 1, 2]


def _brute(rel, idx, S, k, lam, dedup):
    """The specification read aloud, one fp32 scalar at a time."""
    f = np.float32
    lam32 = f(lam)
    oml = f(f(1) - lam32)
    L = len(idx)
    m, picked, out = [f(0)] * L, set(), []
    for _ in range(k):
        best, at = None, -1
        for p in range(L):
            if idx[p] < 0 or p in picked or (dedup is not None and not m[p] < f(dedup)):
                continue
            v = f(f(lam32 * f(rel[p])) - f(oml * m[p]))
            if np.isnan(v):
                v = f(-np.inf)
            if at < 0 or v > best:
                best, at = v, p
        if at < 0:
            out.append((f(-np.inf), -1, f(-np.inf)))
            continue
        out.append((f(rel[at]), int(idx[at]), best))
        picked.add(at)
        m = [max(m[p], f(S[at][p])) for p in range(L)]
    return out


@pytest.fixture(scope="module")
def shortlist():
    rows, _, _, q, _ = dr.products(0)
    rows[5:9] = rows[5]                                              # exact duplicates: the tie rule
    rel, idx = dr.search(rows, q, 40)
    idx[:, -3:] = -1                                                 # pads last
    rel[:, -3:] = -np.inf
    rel[3, 2] = np.nan                                               # a NaN score: its value is -inf, it is picked last
    S = dr.gram(dr.normalized(rows).astype(np.float32), idx).astype(np.float32)
    return rel, idx, S


@pytest.mark.parametrize("dedup", [None, 0.9, 1.0])
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 1.0])
def test_model_equals_the_brute_force_restatement(shortlist, lam, dedup):
    rel, idx, S = shortlist
    for q in range(0, len(idx), 3):
        for k in (1, 10, 40):
            vals, rows, mmr, count, _ = dr.select(rel[q], idx[q], S[q], k, lam, dedup)
            want = _brute(rel[q], idx[q], S[q], k, lam, dedup)
            assert rows.tolist() == [w[1] for w in want], (q, k)
            assert np.array_equal(vals.view(np.uint32), np.array([w[0] for w in want], np.float32).view(np.uint32))
            assert np.array_equal(mmr.view(np.uint32), np.array([w[2] for w in want], np.float32).view(np.uint32))
            assert count == sum(w[1] >= 0 for w in want)


def test_gram_is_symmetric_with_zero_pads_and_uses_fp16_operands():
    rows = dr.normalized(dr.products(1)[0]).astype(np.float32)
    idx = np.array([3, 700, -1, 3, 5000, 12])
    S = dr.gram(rows, idx)
    assert np.array_equal(S, S.T) and (S[2] == 0).all() and (S[:, 4] == 0).all()
    a, b = rows[3].astype(np.float16).astype(np.float64), rows[700].astype(np.float16).astype(np.float64)
    assert S[0, 1] == a @ b and S[0, 3] == a @ a and S[0, 0] == S[3, 3]
    assert S[0, 1] != rows[3].astype(np.float64) @ rows[700].astype(np.float64)
    assert dr.gram(rows, np.stack([idx, idx[::-1]])).shape == (2, 6, 6)
    assert abs(S[0, 0] - 1) < 2.0 ** -10


def test_lam_one_is_the_search_order_and_dedup_is_the_greedy_walk(shortlist):
    rel, idx, S = shortlist
    for q in (0, 5, 11):
        vals, rows, _, count, _ = dr.select(rel[q], idx[q], S[q], 37, 1.0)
        assert rows.tolist() == idx[q, :37].tolist() and count == 37
        assert np.array_equal(vals.view(np.uint32), rel[q, :37].view(np.uint32))
        for t in (0.9, 0.98):
            kept = []
            for p in range(37):                                      # keep a row unless it is within t of a kept row
                if all(S[q][j][p] < np.float32(t) for j in kept):
                    kept.append(p)
            _, rows, _, count, _ = dr.select(rel[q], idx[q], S[q], 37, 1.0, t)
            assert count == len(kept) < 37 and rows[:count].tolist() == idx[q, kept].tolist() and (rows[count:] == -1).all()


def test_follow_judges_every_position_on_its_own(shortlist):
    rel, idx, S = shortlist
    _, own, _, _, _ = dr.select(rel[0], idx[0], S[0], 10, 0.5)
    other = own.copy()
    other[3] = [r for r in idx[0] if r >= 0 and r not in own][0]     # another implementation strays once
    _, judged, _, _, _ = dr.select(rel[0], idx[0], S[0], 10, 0.5, follow=other)
    assert judged[:4].tolist() == own[:4].tolist() and judged[3] != other[3]
    _, again, _, _, _ = dr.select(rel[0], idx[0], S[0], 10, 0.5, follow=own)
    assert again.tolist() == own.tolist()


@pytest.mark.parametrize("seed", SEEDS)
def test_the_fixture_needs_diversification_and_gets_it(seed):
    rows, cat, prod, q, qcat = dr.products(seed)
    g = dr.normalized(rows).astype(np.float32)
    rel, idx = dr.search(rows, q, 100)
    S = dr.gram(g, idx).astype(np.float32)
    plain = idx[:, :10]
    assert dr.distinct(prod, plain).mean() <= 3
    for lam, dedup in ((0.5, None), (1.0, 0.95)):
        picks = np.stack([dr.select(rel[i], idx[i], S[i], 10, lam, dedup)[1] for i in range(len(q))])
        d = dr.distinct(prod, picks)
        print(f"seed {seed} lam={lam} dedup={dedup}: distinct products plain {dr.distinct(prod, plain).mean():.2f}, diversified "
              f"{d.mean():.2f} (min {d.min()})")
        assert (d == 10).all()
        assert (cat[picks] == qcat[:, None]).all()
    assert (cat[plain] == qcat[:, None]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_the_fixture_has_few_near_ties(seed):
    """The premise of the GPU end-to-end test: on these seeds the float64 model alone leaves out at most 5 % of the positions."""
    rows, _, _, q, _ = dr.products(seed)
    g = dr.normalized(rows).astype(np.float32)
    rel, idx = dr.search(rows, q, 100)
    S = dr.gram(g, idx)
    tol = dr.gram_tol(rows.shape[1])
    for lam, dedup in ((0.3, None), (0.7, None), (0.7, 0.9)):
        near = np.stack([dr.near_ties(dr.select(rel[i], idx[i], S[i], 10, lam, dedup, dtype=np.float64)[4], tol) for i in range(len(q))])
        print(f"seed {seed} lam={lam} dedup={dedup}: {near.mean():.3f} of the positions are near-ties")
        assert near.mean() <= 0.05
