"""Result diversification on the GPU against the NumPy model (tests/diversify_ref.py), stage by stage on the GPU's own inputs: the
shortlist Gram matrix (within the derived fp32 accumulation bound of the float64 reference, pads exactly 0, bit-symmetric, the
bits of a pair of rows the same wherever it occurs), the greedy selection (bit for bit against the model's fp32 recipe),
``Gallery.diversify`` end to end on fp32, fp16 and prepared galleries, bit-for-bit properties, and what it is for: distinct
products on the ``products`` fixture through the public API."""
import functools

import numpy as np
import pytest
import torch

import diversify_ref as dr
import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import diversify as D
from imageretrievalresearch_amd import rerank as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, ROWS = 37, 1200
KINDS = ["fp32", "fp16", "prepared"]
# (L, D): one slot; one short of, exactly and one past a wave and a 64-slot tile; five tiles a side with a 1-slot tail; the limit.
# D = 7 and 70 take the scalar fp32 loads and the masked fp16 tail, 64 / 256 / 32 the vector loads
CASES = [(1, 7), (63, 70), (64, 64), (65, 256), (257, 70), (1024, 32)]
LAMS, DEDUPS = [0.0, 0.3, 0.7, 1.0], [None, 0.9, 1.0]
SEEDS = [0, 1, 2]                                    # tests/test_diversify_ref.py: at most 5 % near-ties on the model alone


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(f"i{a.dtype.itemsize}")


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(_np(x)), _bits(_np(y)))
                                    for x, y in zip(a, b))


def _gallery(x, kind):
    x = torch.as_tensor(x).to(DEV)
    if kind == "fp16":
        return M.Gallery(x.shape[1], DEV, dtype=torch.float16).add(x)
    gal = M.Gallery(x.shape[1], DEV).add(x)
    return gal.prepare() if kind == "prepared" else gal


@functools.lru_cache(maxsize=None)
def _clustered(dim):
    """(rows (1200, dim) of 20 clusters with a block of exactly duplicated rows (10 .. 17), 37 queries: noisy copies of rows, the
    first four of the duplicated one)."""
    g = torch.Generator().manual_seed(11 + dim)
    centers = torch.randn(20, dim, generator=g)
    x = centers[torch.randint(0, 20, (ROWS,), generator=g)] + torch.randn(ROWS, dim, generator=g)
    x[10:18] = x[10]
    own = torch.randint(0, ROWS, (Q,), generator=g)
    own[:4] = 10
    q = x[own] + 0.3 * torch.randn(Q, dim, generator=g)
    return x, q, own


@functools.lru_cache(maxsize=None)
def _clustered_gallery(dim, kind, rows=ROWS):
    return _gallery(_clustered(dim)[0][:rows], kind)


@functools.lru_cache(maxsize=None)
def _gram64(dim, kind, rows=ROWS):
    """The float64 Gram matrix of the whole gallery's fp16 operands: every shortlist's reference is a gather from it."""
    x = dr.f16_rows(_np(_clustered_gallery(dim, kind, rows).data))
    return x @ x.T


@functools.lru_cache(maxsize=None)
def _run(kind, L, dim):
    """The GPU's own shortlists of one gallery kind and (L, D) and their Gram matrices, kept on the device and never changed."""
    gal = _clustered_gallery(dim, kind)
    sv, si = K._shortlist_search(gal, _clustered(dim)[1].to(DEV), L, None)
    sv, si = sv.contiguous(), si.contiguous()
    return sv, si, D._dv_gram(gal, si)


def _want(G64, rows):
    ok = rows >= 0
    r = np.where(ok, rows, 0)
    return G64[np.ix_(r, r)] * (ok[:, None] & ok[None, :])


def _check_gram(S, si, G64, dim, what):
    assert S.dtype == np.float32 and S.shape == si.shape + si.shape[1:]
    worst = 0.0
    for q in range(len(si)):
        worst = max(worst, float(np.abs(S[q] - _want(G64, si[q])).max()))
        pad = si[q] < 0
        assert (S[q][pad] == 0).all() and (S[q][:, pad] == 0).all()
        assert np.array_equal(_bits(S[q]), _bits(S[q].T))               # bit-symmetric
    tol = dr.gram_tol(dim)
    print(f"gram {what} L={si.shape[1]} D={dim}: max |S - float64| {worst:.3e} = {worst / tol:.3f} of the bound {tol:.3e}")
    assert worst <= tol


# ---------------------------------------------------------------------------------------------- the Gram stage
@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_gram_stage(kind, case):
    L, dim = case
    _, si, S = _run(kind, L, dim)
    si = _np(si)
    assert (si >= 0).all()
    _check_gram(_np(S), si, _gram64(dim, kind), dim, kind)
    if L >= 63:                                                          # the duplicated block is in the first queries' shortlists
        assert np.isin(np.arange(10, 18), si[0]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_gram_stage_with_a_pad_and_rows_outside_the_gallery(kind):
    """Every row of a 257-row gallery but the query's own: L = rows, so the last slot is the pad of ``exclude``; then the same
    shortlists with an index past the gallery, which counts as a pad too."""
    dim, rows = 70, 257
    gal = _clustered_gallery(dim, kind, rows)
    own = torch.arange(0, rows, 7, device=DEV)[:Q]
    _, si = K._shortlist_search(gal, gal.data[own].float(), rows, own)
    si = si.contiguous()
    assert (si[:, -1] == -1).all() and (si[:, :-1] >= 0).all()
    _check_gram(_np(D._dv_gram(gal, si)), _np(si), _gram64(dim, kind, rows), dim, f"{kind} with a pad")
    si[:, 3] = rows
    si[:, 100] = -5
    S = _np(D._dv_gram(gal, si))
    assert (S[:, 3] == 0).all() and (S[:, :, 3] == 0).all() and (S[:, 100] == 0).all() and (S[:, :, 100] == 0).all()
    _check_gram(S, np.where(_np(si) == rows, -1, _np(si)), _gram64(dim, kind, rows), dim, f"{kind} with rows outside the gallery")


@pytest.mark.parametrize("kind", KINDS)
def test_a_pair_of_rows_has_the_same_bits_wherever_it_occurs(kind):
    """Over the shortlists of 37 queries at L = 65 and L = 257 on one gallery: every unordered pair of rows, in whichever query,
    slots, tile or L it occurs, and whichever of the two comes first, carries one bit pattern."""
    keys, bits, where = [], [], []
    for L in (65, 257):
        _, si, S = _run(kind, L, 70)
        si, S = _np(si), _np(S)
        a, b = np.broadcast_arrays(si[:, :, None], si[:, None, :])
        keys.append((np.minimum(a, b) * ROWS + np.maximum(a, b)).ravel())
        bits.append(_bits(S).ravel())
        where.append(np.broadcast_to(np.arange(Q)[:, None, None] + 1000 * (L == 257), S.shape).ravel())
    keys, bits, where = np.concatenate(keys), np.concatenate(bits), np.concatenate(where)
    order = np.argsort(keys, kind="stable")
    keys, bits, where = keys[order], bits[order], where[order]
    again = keys[1:] == keys[:-1]
    assert (bits[1:][again] == bits[:-1][again]).all()
    shared = again & (where[1:] != where[:-1])
    print(f"{kind}: {again.sum()} repeated occurrences of a pair, {shared.sum()} of them across queries or shortlist lengths")
    assert shared.sum() > 10000                                          # the case has what it is about


# ---------------------------------------------------------------------------------------------- the select stage
def _queries_of(L):
    return range(Q) if L <= 65 else (0, 1, 2, 3, 20, 36)                 # the long shortlists: fewer queries for the model to walk


@pytest.mark.parametrize("dedup", DEDUPS)
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("kind, case", [("fp32", c) for c in CASES] + [("fp16", CASES[3]), ("prepared", CASES[1])], ids=str)
def test_select_stage(kind, case, lam, dedup):
    """Fed the GPU's own scores, rows and Gram matrices: rows, cosine scores, MMR values and counts bit for bit with the model.
    One wave (L <= 64), two, five and sixteen waves; the duplicated block ties; dedup=0.9 with k = L runs out of slots."""
    L, dim = case
    sv, si, S = _run(kind, L, dim)
    qs = list(_queries_of(L))
    pick = torch.tensor(qs, device=DEV)
    sv, si, S = sv[pick].contiguous(), si[pick].contiguous(), S[pick].contiguous()
    if L == 257:                                                         # pads last
        si, sv = si.clone(), sv.clone()
        si[:, -2:], sv[:, -2:] = -1, float("-inf")
    svn, sin, Sn = _np(sv), _np(si), _np(S)
    ran_out = 0
    for k in sorted({1, min(10, L), L}):
        got = [_np(t) for t in D._dv_select(sv, si, S, k, lam, dedup)]
        assert [g.dtype for g in got] == [np.float32, np.int64, np.float32, np.int32]
        for n in range(len(qs)):
            vals, rows, mmr, count, _ = dr.select(svn[n], sin[n], Sn[n], k, lam, dedup)
            assert np.array_equal(got[1][n], rows), (kind, case, lam, dedup, k, qs[n])
            assert np.array_equal(_bits(got[0][n]), _bits(vals)) and np.array_equal(_bits(got[2][n]), _bits(mmr))
            assert got[3][n] == count
            ran_out += count < k
    if dedup == 0.9 and L >= 63:
        assert ran_out > 0


def test_select_ties_go_to_the_lower_position():
    """The duplicated rows tie in score and in every Gram entry: with lam = 0 every unpicked slot ties at each pick."""
    sv, si, S = _run("fp32", 65, 256)
    _, rows, _, _ = D._dv_select(sv, si, S, 3, 0.0)
    assert torch.equal(rows[:, 0], si[:, 0])                             # all values are 0: the first slot
    dup = torch.isin(si[0], torch.arange(10, 18, device=DEV)).nonzero().flatten()
    assert len(dup) == 8
    v, r, _, c = D._dv_select(sv[:1], si[:1], S[:1], 65, 1.0, 0.999)
    assert int(c) < 65 and torch.isin(r[0], si[0][dup]).sum() == 1 and si[0][dup[0]] in r[0]


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("kind", KINDS)
def test_diversify_equals_the_staged_calls(kind):
    gal, q = _clustered_gallery(70, kind), _clustered(70)[1].to(DEV)
    for k, L, lam, dedup in ((10, 257, 0.7, None), (10, None, 0.3, 0.9), (63, 63, 0.5, 0.95), (1, 1, 0.7, None)):
        out = gal.diversify(q, k, lam=lam, dedup=dedup, shortlist=L, stats=True)
        L = 100 if L is None else L
        sv, si = K._shortlist_search(gal, q, L, None)
        sv, si = sv.contiguous(), si.contiguous()
        assert _same(out, D._dv_select(sv, si, D._dv_gram(gal, si), k, lam, dedup))
        assert _same(out[:2], gal.diversify(q, k, lam=lam, dedup=dedup, shortlist=L))


@functools.lru_cache(maxsize=None)
def _products(seed, kind):
    rows, cat, prod, q, qcat = dr.products(seed)
    return _gallery(rows, kind), torch.from_numpy(q).to(DEV), cat, prod, qcat


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", KINDS)
def test_diversify_against_the_float64_model(kind, seed):
    """The model walks the GPU's own shortlist in float64 and is told the GPU's pick after each of its own, so that every position
    is judged on its own.  Two values differ between fp32 and float64 by at most 2 (oml * tol + 1.5 * 2^-24) < 2 tol for
    oml <= 0.7 and D = 64 (the Gram bound, and three roundings of numbers below 1): positions the model wins by less than twice
    the Gram tolerance are left out, at most 5 % of them."""
    gal, q, *_ = _products(seed, kind)
    sv, si = K._shortlist_search(gal, q, 100, None)
    svn, sin = _np(sv), _np(si)
    rows = _np(gal.data)
    tol = dr.gram_tol(64)
    for lam, dedup in ((0.3, None), (0.7, None), (0.7, 0.9)):
        _, idx = gal.diversify(q, 10, lam=lam, dedup=dedup, shortlist=100)
        idx = _np(idx)
        judged = left_out = 0
        for n in range(len(idx)):
            _, want, _, _, margins = dr.select(svn[n], sin[n], dr.gram(rows, sin[n]), 10, lam, dedup, dtype=np.float64, follow=idx[n])
            near = dr.near_ties(margins, tol)
            assert np.array_equal(idx[n][~near], want[~near]), (kind, seed, lam, dedup, n)
            judged, left_out = judged + (~near).sum(), left_out + near.sum()
        print(f"{kind} seed {seed} lam={lam} dedup={dedup}: {judged} positions equal, {left_out} near-ties left out")
        assert left_out <= 0.05 * (judged + left_out)


# ---------------------------------------------------------------------------------------------- properties, bit for bit
KW = dict(lam=0.6, dedup=0.97, shortlist=120)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_size_blocking_and_repetition_do_not_change_the_bits(kind):
    gal, q = _clustered_gallery(70, kind), _clustered(70)[1].to(DEV)
    own = _clustered(70)[2].to(DEV)
    full = gal.diversify(q, 10, exclude=own, stats=True, **KW)
    assert _same(full, gal.diversify(q, 10, exclude=own, stats=True, **KW))
    assert _same(full, gal.diversify(q, 10, exclude=own, stats=True, block=8, **KW))
    assert _same(full, gal.diversify(q, 10, exclude=own, stats=True, block=1000, **KW))
    for n in (1, 4, 5):
        part = gal.diversify(q[:n], 10, exclude=own[:n], stats=True, **KW)
        assert _same(part, [t[:n] for t in full]), n
    alone = gal.diversify(q[20:21], 10, exclude=own[20:21], stats=True, block=1, **KW)
    assert _same(alone, [t[20:21] for t in full])
    assert not (_np(full[1]) == _np(own)[:, None]).any()


def test_idx_offset_shifts_the_indices_and_exclude():
    gal, (_, q, own) = _clustered_gallery(70, "fp32"), _clustered(70)
    q, own = q.to(DEV), own.to(DEV)
    v0, i0, m0, c0 = gal.diversify(q, 120, exclude=own, stats=True, **KW)
    v1, i1, m1, c1 = gal.diversify(q, 120, exclude=own + 1000, idx_offset=1000, stats=True, **KW)
    assert _same((v0, m0, c0), (v1, m1, c1)) and torch.equal(torch.where(i0 >= 0, i0 + 1000, i0), i1)
    assert (c0[:4] < 120).all() and (i0[:4, -1] == -1).all() and torch.isneginf(v0[i0 < 0]).all()   # the duplicates: out of slots


@pytest.mark.parametrize("kind", KINDS)
def test_lam_one_without_dedup_is_the_search(kind):
    gal, q = _clustered_gallery(70, kind), _clustered(70)[1].to(DEV)
    for k, L in ((10, 100), (65, 65), (7, 300)):
        v, i = gal.search(q, L)
        got = gal.diversify(q, k, lam=1.0, shortlist=L, stats=True)
        assert _same(got[:2], (v[:, :k].contiguous(), i[:, :k].contiguous()))
        assert (got[3] == k).all() and _same(got[2:3], (v[:, :k].contiguous(),))          # lam = 1: the MMR value is the score


def test_gallery_diversify_equals_mmr_rerank_and_empty_batches():
    x, q, own = _clustered(70)
    gal, x, q, own = _clustered_gallery(70, "fp32"), x.to(DEV), q.to(DEV), own.to(DEV)
    assert _same(gal.diversify(q, 10, exclude=own, stats=True, **KW), M.mmr_rerank(q, x, 10, exclude=own, stats=True, **KW))
    assert _same(gal.diversify(q, 7), D.mmr_rerank(q, x, 7))
    out = gal.diversify(q[:0], 6, stats=True)
    assert [tuple(t.shape) for t in out] == [(0, 6), (0, 6), (0, 6), (0,)]
    assert [t.dtype for t in out] == [torch.float32, torch.int64, torch.float32, torch.int32]
    assert [tuple(t.shape) for t in M.mmr_rerank(q[:0], x, 6)] == [(0, 6), (0, 6)]
    e = D._dv_gram(gal, torch.zeros((0, 5), dtype=torch.int64, device=DEV))
    assert e.shape == (0, 5, 5) and e.dtype == torch.float32


# ---------------------------------------------------------------------------------------------- what it is for
@pytest.mark.parametrize("seed", SEEDS[:2])
@pytest.mark.parametrize("kind", KINDS)
def test_distinct_products_through_the_public_api(kind, seed):
    gal, q, cat, prod, qcat = _products(seed, kind)
    plain = _np(gal.search(q, 10)[1])
    assert dr.distinct(prod, plain).mean() <= 3 and (cat[plain] == qcat[:, None]).all()
    for kw in (dict(lam=0.5), dict(lam=1.0, dedup=0.95)):
        idx = _np(gal.diversify(q, 10, **kw)[1])
        d = dr.distinct(prod, idx)
        print(f"{kind} seed {seed} {kw}: distinct products in the top-10: plain {dr.distinct(prod, plain).mean():.2f}, diversified "
              f"{d.mean():.2f} (min {d.min()})")
        assert (d == 10).all() and (cat[idx] == qcat[:, None]).all()
