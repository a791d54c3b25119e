"""``RegionGallery`` / ``maxsim`` on the GPU against the float64 model of tests/regional_ref.py.

The model is fed the codes the device stored (``rg.data``, ``rg.query_codes``): the stored codes are checked on their own - bit
for bit against the fp16 ``Gallery`` and within one fp16 unit of the model's float64 rounding - so the score tests measure the
score kernel alone, with the derived tolerance ``tol = (dim + Rq) * 2^-24 * max(1, sum |w|)`` (regional_ref.tol).  A match must
equal the model's wherever the model's gap between best and second best exceeds 2 tol.  Shapes are the smallest that reach each
branch: every 16-row tile count of either side, ld 64 / 128 / 256 with a zero tail, the resident and the chunked query, lists
with pads, and one retrieval fixture."""
import functools

import numpy as np
import pytest
import torch

import regional_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _M():
    import imageretrievalresearch_amd as M
    return M


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _build(g, q):
    """(rg, query tensor, gh, qh): the gallery of regions g, and the codes the device keeps for both sides, on the host."""
    rg = _M().RegionGallery(g.shape[2], g.shape[1], DEV, capacity=g.shape[0]).add(_dev(g))
    qt = _dev(q)
    dim = g.shape[2]
    return rg, qt, rg.data.cpu().numpy(), rg.query_codes(qt)[:, :, :dim].cpu().numpy()


def _check(got, qh, gh, idx=None, weights=None, matches=None, what=""):
    """Scores within tol of the model's; pads -inf; matches equal wherever the model's gap exceeds 2 tol.  Returns the share of
    match entries skipped for a smaller gap."""
    dim, Rq = qh.shape[2], qh.shape[1]
    t = RR.tol(dim, Rq, weights)
    want, wa, gap = RR.scores(qh, gh, idx, weights)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, what
    pad = np.isneginf(want)
    assert (np.isneginf(got) == pad).all(), what
    err = np.abs(got[~pad] - want[~pad]).max() if (~pad).any() else 0.0
    print(f"{what}: max |score - model| = {err:.3g}, tol {t:.3g}")
    assert err <= t, (what, err, t)
    if matches is None:
        return 0.0
    ma = matches.cpu().numpy()
    assert ma.dtype == np.int32 and ma.shape == wa.shape
    assert (ma[pad] == -1).all()
    sure = gap > 2 * t
    assert (ma[sure] == wa[sure]).all(), what
    assert ((ma[~pad] >= 0) & (ma[~pad] < gh.shape[1])).all()
    return float((~sure).mean())


def _lists(seed, Q, L, G):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, G, (Q, L))
    idx[:: (2 if L == 1 else 1), 0] = -1                         # a pad in front (a one-slot list: of every other query)
    if L > 2:
        idx[:, L // 2] = -1                                      # in the middle
        idx[:, -1] = -1                                          # at the end
    if L > 4:
        idx[:, 3] = idx[:, 1]                                    # a row twice
    if L > 6:
        idx[0, 5] = G + 3                                        # outside the gallery: treated as a pad, nothing is read
    return idx


# ------------------------------------------------------------------------------------------------------ tiles and pads
@pytest.mark.parametrize("R, Rq, dim, rows", [(1, 1, 8, 50), (3, 3, 72, 33), (14, 14, 200, 50), (16, 17, 8, 20), (17, 3, 72, 20),
                                             (33, 14, 200, 9), (64, 64, 72, 7), (14, 64, 8, 11), (64, 1, 200, 6), (33, 33, 8, 5)])
def test_tile_and_pad_edges(R, Rq, dim, rows):
    g, q = RR.random_regions(R * 100 + Rq, rows, R, dim), RR.random_regions(7, 5, Rq, dim)
    rg, qt, gh, qh = _build(g, q)
    ld = (dim + 63) // 64 * 64
    assert tuple(rg._buf.shape[1:]) == (R, ld) and not rg._buf[:rows, :, dim:].any()         # the zero tail of every row
    s, m = rg.scores(qt, matches=True)
    _check(s, qh, gh, None, None, m, f"R={R} Rq={Rq} dim={dim} every row")
    idx = _lists(3, 5, min(rows, 9), rows)
    s, m = rg.scores(qt, _dev(idx), matches=True)
    _check(s, qh, gh, idx, None, m, f"R={R} Rq={Rq} dim={dim} list")
    assert torch.equal(rg.scores(qt, _dev(idx)), s)                                           # without matches: the same bits
    assert torch.equal(_M().maxsim(qt, _dev(g)), rg.scores(qt))                               # the wrapper: a temporary gallery


@pytest.mark.parametrize("R, Rq, dim, rows", [(64, 64, 2560, 5), (14, 14, 1536, 12), (14, 64, 1536, 6), (3, 17, 1100, 6)])
def test_long_rows_resident_and_chunked(R, Rq, dim, rows):
    """Rq = 14 at 1536 keeps the whole query in LDS; 64 regions of 2560 (327 KB) or 1536, and 32 padded rows of 1152, go through it
    in chunks of d with the accumulators in registers."""
    from imageretrievalresearch_amd import regional as RG
    full = (Rq + 15) // 16 * 16 * ((dim + 63) // 64 * 64 + 8) * 2
    assert (RG.lds_bytes(Rq, dim) == full) == (Rq == 14)
    g, q = RR.random_regions(dim + R, rows, R, dim), RR.random_regions(dim + 1, 3, Rq, dim)
    rg, qt, gh, qh = _build(g, q)
    s, m = rg.scores(qt, matches=True)
    _check(s, qh, gh, None, None, m, f"R={R} Rq={Rq} dim={dim}")
    idx = _lists(5, 3, 9, rows)                                  # more slots than waves: a chunked query is staged again
    s2, m2 = rg.scores(qt, _dev(idx), matches=True)
    _check(s2, qh, gh, idx, None, m2, f"R={R} Rq={Rq} dim={dim} list")


def test_all_negative_scores_keep_pad_regions_out():
    """Every s[i][j] < 0 with 13 pad columns and 13 pad rows in the tile: a zero pad column would win every maximum."""
    q, g = RR.all_negative(11, 5, 20, 3, 40)
    rg, qt, gh, qh = _build(g, q)
    assert RR.pair_tables(qh, gh).max() < -0.5
    s, m = rg.scores(qt, matches=True)
    want = RR.scores(qh, gh)[0]
    assert want.max() < -0.5 and float(s.max()) < -0.5
    _check(s, qh, gh, None, None, m, "all negative")
    w = torch.full((5, 3), 0.5, device=DEV)
    assert float(rg.scores(qt, weights=w).max()) < -0.75


# ------------------------------------------------------------------------------------------------------ lists
@functools.lru_cache(maxsize=None)
def _small():
    g, q = RR.random_regions(21, 50, 14, 72), RR.random_regions(22, 37, 5, 72)
    return _build(g, q)


@pytest.mark.parametrize("L, Q", [(1, 37), (7, 5), (100, 1), (1024, 5), (1024, 37), (7, 1)])
def test_lists_with_pads_and_repeats(L, Q):
    rg, qt, gh, qh = _small()
    idx = _lists(L + Q, Q, L, 50)
    s, m = rg.scores(qt[:Q], _dev(idx), matches=True)
    _check(s, qh[:Q], gh, idx, None, m, f"L={L} Q={Q}")
    if L > 4:
        assert torch.equal(s[:, 3], s[:, 1]) and torch.equal(m[:, 3], m[:, 1])              # the row that stands twice
    every = rg.scores(qt[:Q])
    assert every.shape == (Q, 50)
    real = torch.from_numpy(((idx >= 0) & (idx < 50))).to(DEV)
    assert torch.equal(s[real], every.gather(1, _dev(idx).clamp(0, 49))[real])             # the bits of idx=None


def test_a_pair_gives_the_same_bits_wherever_it_stands():
    rg, qt, gh, qh = _small()
    q0, r0 = 20, 31
    one, m_one = rg.scores(qt[q0:q0 + 1], _dev(np.array([[r0]])), matches=True)
    bits = one.view(torch.int32)[0, 0]
    idx = np.random.default_rng(1).integers(0, 50, (37, 1024))
    slots = (0, 513, 1023)
    idx[:, slots] = r0
    many, m_many = rg.scores(qt, _dev(idx), matches=True)
    for p in slots:
        assert many.view(torch.int32)[q0, p] == bits and torch.equal(m_many[q0, p], m_one[0, 0])
    alone, m_alone = rg.scores(qt[q0:q0 + 1], _dev(idx[q0:q0 + 1]), matches=True)
    assert torch.equal(alone.view(torch.int32)[0], many.view(torch.int32)[q0]) and torch.equal(m_alone[0], m_many[q0])
    for qs in (slice(q0, q0 + 1), slice(0, 37)):
        every, m_every = rg.scores(qt[qs], matches=True)
        row = 0 if qs.start else q0
        assert every.view(torch.int32)[row, r0] == bits and torch.equal(m_every[row, r0], m_one[0, 0])
    few, m_few = rg.scores(qt[q0 - 2:q0 + 3], _dev(np.full((5, 7), r0)), matches=True)
    assert (few.view(torch.int32)[2] == bits).all() and torch.equal(m_few[2, 6], m_one[0, 0])


def test_weights_zero_negative_and_unnormalised():
    rg, qt, gh, qh = _small()
    rng = np.random.default_rng(9)
    w = rng.standard_normal((37, 5)).astype(np.float32) * 2      # negative ones, sums far from 1
    w[::3, 1] = 0
    w[1, :] = 0                                                  # a query without any region
    w[2, 2:] = 0                                                 # a ragged query: two regions
    idx = _lists(4, 37, 20, 50)
    s, m = rg.scores(qt, _dev(idx), weights=_dev(w), matches=True)
    _check(s, qh, gh, idx, w, m, "weights")
    real = (idx[1] >= 0) & (idx[1] < 50)
    assert (s[1].cpu().numpy()[real] == 0).all()
    s2 = rg.scores(qt[2:3, :2], _dev(idx[2:3]), weights=_dev(w[2:3, :2]))                   # the ragged query as a 2-region one:
    assert torch.equal(s2, s[2:3])                                                           # a zero weight adds exactly nothing
    unit = torch.full((37, 5), float(np.float32(1) / np.float32(5)), device=DEV)
    assert torch.equal(rg.scores(qt, _dev(idx), weights=unit), rg.scores(qt, _dev(idx)))     # the default weight, bit for bit


def test_identical_regions_match_the_lower_one():
    g, q = RR.random_regions(31, 30, 20, 72), RR.random_regions(32, 9, 6, 72)
    g[:, 17] = g[:, 2]
    g[:, 9] = g[:, 2]
    g[::2, 1] = g[::2, 0]
    rg, qt, gh, qh = _build(g, q)
    assert (gh[:, 17] == gh[:, 2]).all() and (gh[:, 9] == gh[:, 2]).all()
    s, m = rg.scores(qt, matches=True)
    ma = m.cpu().numpy()
    assert not np.isin(ma, (9, 17)).any() and not (ma[:, ::2] == 1).any()                   # equal bits: the lower region, exactly
    wa = RR.scores(qh, gh)[1]
    assert (wa == 2).mean() > 0.05 and (ma == 2).mean() > 0.05                               # and the tie does occur
    _check(s, qh, gh, None, None, m, "identical regions")


# ------------------------------------------------------------------------------------------------------ storage
def test_codes_are_the_fp16_gallery_bits_and_pooled_is_the_sum_of_regions():
    M = _M()
    from imageretrievalresearch_amd.aggregate import _sum_regions
    g = RR.random_regions(41, 23, 14, 200)
    labels = torch.arange(23, device=DEV) % 4
    rg = M.RegionGallery(200, 14, DEV).add(_dev(g[:10]), labels[:10]).add(_dev(g[10:]).half(), labels[10:])   # grows; fp16 input
    flat = M.Gallery(200, DEV, dtype=torch.float16).add(_dev(g[:10]).view(-1, 200)).add(_dev(g[10:]).half().float().view(-1, 200))
    assert len(rg) == 23 and rg.nbytes == rg._buf.shape[0] * 14 * 256 * 2
    assert torch.equal(rg.data.reshape(-1, 200).view(torch.int16), flat.data.view(torch.int16))
    assert torch.equal(rg.labels, labels)
    model = RR.codes(g[:10]).astype(np.float64)
    got = rg.data[:10].cpu().numpy().astype(np.float64)
    assert (np.abs(got - model) <= 2.0 ** -10 * np.abs(model) + 2.0 ** -24).all()             # one fp16 unit: the norm is fp32
    qc = rg.query_codes(_dev(g[:3, :5]).bfloat16())
    assert qc.shape == (3, 5, 256) and qc.dtype == torch.float16 and not qc[:, :, 200:].any()
    want = _sum_regions(rg.data.float().contiguous(), True, rg.eps)
    for dt in (torch.float32, torch.float16):
        p = rg.pooled(dt)
        assert isinstance(p, M.Gallery) and len(p) == 23 and p.dtype == dt and torch.equal(p.labels, labels)
        assert torch.equal(p.data, want if dt == torch.float32 else want.half())
    assert np.abs(want.cpu().numpy() - RR.pooled(rg.data.cpu().numpy())).max() < 1e-5


# ------------------------------------------------------------------------------------------------------ search and rerank
def _check_topk(vals, idx, sc, k, t, idx_offset, what):
    """vals / idx (Q, k) against the model's scores sc (Q, G) of LOCAL rows (-inf: not eligible)."""
    vals, idx = vals.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    kth = -np.sort(-sc, axis=1)[:, k - 1]
    for q in range(sc.shape[0]):
        real = idx[q] >= 0
        n = int(real.sum())
        assert real[:n].all() and np.isneginf(vals[q, n:]).all(), (what, q)                   # pads come last
        assert n == min(k, int(np.isfinite(sc[q]).sum())), (what, q)
        loc = idx[q, :n] - idx_offset
        assert len(set(loc.tolist())) == n and ((loc >= 0) & (loc < sc.shape[1])).all(), (what, q)
        assert np.abs(vals[q, :n] - sc[q, loc]).max() <= t, (what, q)
        assert (np.diff(vals[q, :n]) <= 0).all() and (vals[q, :n] >= kth[q] - 2 * t).all(), (what, q)


@functools.lru_cache(maxsize=None)
def _ranked():
    g, q = RR.random_regions(51, 300, 5, 72), RR.random_regions(52, 6, 4, 72)
    return _build(g, q)


def test_search_against_the_model():
    rg, qt, gh, qh = _ranked()
    t = RR.tol(72, 4)
    v, i = rg.search(qt, 10)
    _check_topk(v, i, RR.scores(qh, gh)[0], 10, t, 0, "search")
    ex = np.array([1003, 1000, 1299, 5, 2000, 1150])
    w = np.random.default_rng(3).random((6, 4)).astype(np.float32)
    v, i = rg.search(qt, 300, weights=_dev(w), exclude=_dev(ex), idx_offset=1000)
    sc = RR.search(qh, gh, 300, w, ex, 1000)[2]
    _check_topk(v, i, sc, 300, RR.tol(72, 4, w), 1000, "search with exclude")
    got = i.cpu().numpy()
    for q, e in enumerate(ex):
        assert e not in got[q] and (got[q, -1] == -1) == (1000 <= e < 1300)
    v1, i1 = rg.search(qt[:1], 3)
    assert torch.equal(v1, rg.search(qt, 3)[0][:1]) and torch.equal(i1, rg.search(qt, 3)[1][:1])


@pytest.mark.parametrize("Q, k, shortlist, dtype", [(6, 10, 40, torch.float32), (2, 5, None, torch.float16), (6, 300, 300, torch.float32)])
def test_rerank_against_the_model(Q, k, shortlist, dtype):
    from imageretrievalresearch_amd.rerank import _shortlist_search
    M = _M()
    rg, qt, gh, qh = _ranked()
    qt, qh = qt[:Q], qh[:Q]
    gal = rg.pooled(dtype)
    qg = M.RegionGallery(72, 4, DEV).add(qt).pooled().data                                  # the queries' own pooled rows
    L = min(300, max(k, 100)) if shortlist is None else shortlist
    ex = np.array([1003, 1000, 1299, 5, 2000, 1150])[:Q]
    for kw, exl in ((dict(), None), (dict(exclude=_dev(ex), idx_offset=1000), _dev(ex) - 1000)):
        off = kw.get("idx_offset", 0)
        si = _shortlist_search(gal, qg, L, exl)[1].cpu().numpy()
        v, i, m = rg.rerank(gal, qg, qt, k, shortlist=shortlist, matches=True, **kw)
        assert v.shape == (Q, k) and i.dtype == torch.int64 and m.shape == (Q, k, 4)
        sc = np.full((Q, 300), -np.inf)
        full = RR.scores(qh, gh)[0]
        for q in range(Q):
            rows = si[q][si[q] >= 0]
            sc[q, rows] = full[q, rows]
        _check_topk(v, i, sc, k, RR.tol(72, 4), off, f"rerank {kw}")
        wv, wi, wm, _ = RR.rerank(qh, gh, si, k, idx_offset=off)
        same = i.cpu().numpy() == wi
        assert same.mean() > 0.95 and (m.cpu().numpy()[same] == wm[same]).mean() > 0.99       # exact order but for near-ties
        v2, i2 = rg.rerank(gal, qg, qt, k, shortlist=shortlist, **kw)
        assert torch.equal(v2, v) and torch.equal(i2, i)
        if exl is not None:
            for q, e in enumerate(ex):
                assert e not in i.cpu().numpy()[q]


# ------------------------------------------------------------------------------------------------------ retrieval value
@functools.lru_cache(maxsize=None)
def _planted():
    g, gl, q, ql = RR.planted_parts(dim=128)
    rg, qt, gh, qh = _build(g, q)
    return rg, qt, gh, qh, gl, ql


def test_retrieval_value_equals_the_models():
    """The planted-part fixture (dim 128, R = Rq = 14, 30 classes x 20 images, 60 queries): precision@1 of ``search`` and of ``rerank``
    over ``pooled()`` at a shortlist of 100 equal the model's, which tests/test_regional_ref.py holds to >= 0.95 regional and
    <= 0.30 pooled."""
    M = _M()
    rg, qt, gh, qh, gl, ql = _planted()
    want_search = RR.precision_at_1(RR.search(qh, gh, 1)[1][:, 0], ql, gl)
    short = RR.global_shortlist(RR.pooled(qh), RR.pooled(gh), 100)
    want_rerank = RR.precision_at_1(RR.rerank(qh, gh, short, 1)[1][:, 0], ql, gl)
    want_pooled = RR.precision_at_1(short[:, 0], ql, gl)
    gal = rg.pooled()
    qg = M.RegionGallery(128, 14, DEV).add(qt).pooled().data
    got_search = RR.precision_at_1(rg.search(qt, 1)[1].cpu().numpy()[:, 0], ql, gl)
    got_rerank = RR.precision_at_1(rg.rerank(gal, qg, qt, 1, shortlist=100)[1].cpu().numpy()[:, 0], ql, gl)
    got_pooled = RR.precision_at_1(gal.search(qg, 1)[1].cpu().numpy()[:, 0], ql, gl)
    print(f"precision@1 search {got_search:.3f} (model {want_search:.3f}), rerank {got_rerank:.3f} (model {want_rerank:.3f}), "
          f"pooled rows {got_pooled:.3f} (model {want_pooled:.3f})")
    assert got_search == want_search and got_rerank == want_rerank
    assert want_search >= 0.95 and want_rerank >= 0.95 and got_pooled <= 0.30


def test_matches_on_the_fixture_and_the_share_left_out():
    rg, qt, gh, qh, gl, ql = _planted()
    s, m = rg.scores(qt, matches=True)
    skipped = _check(s, qh, gh, None, None, m, "planted parts")
    print(f"match entries left out for a gap <= 2 tol: {100 * skipped:.3f} %")
    assert skipped <= 0.01
