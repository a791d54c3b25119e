"""Asymmetric binary search on the GPU - int8 query codes against the gallery's sign bits on the i8 MFMA - against the NumPy
model of the contract (binary_asym_ref.py) BIT FOR BIT: the query quantiser, the weighted distances, every search path, ties,
the k > 8 route, the key packing at the largest distance, the refined search, the recall condition and the side streams.
Integer arithmetic and one fp32 division: no tolerance and no tie slack anywhere."""
import numpy as np
import pytest
import torch

import binary_asym_ref as A
import binary_ref as R
import imageretrievalresearch_amd as M
import stream_harness as H
from imageretrievalresearch_amd import Gallery, IVFIndex, binary
from imageretrievalresearch_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_ASYM, FUSED, BITONIC = 11, 0x100, 0x200
CHUNK = binary.SCAN_CHUNK
AQB = 2 * binary.ASYM_QUERY_BLOCK                                   # two query blocks of the asymmetric scan
CODE_DIMS = [1, 31, 32, 33, 63, 64, 65, 96, 128, 130, 1000, 1536, 2560]
DIMS = [1, 31, 32, 33, 96, 128, 130, 1000, 1536, 2560]              # the dims of test_binary_gpu.py
SIZES = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
GMAX = 2 * CHUNK + 1
QS = [1, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, AQB + 1]         # around the 32-query A tiles; one past one and two blocks
NQ = AQB + 1
KS = [1, 3, 8, 9, 150, 1024]


def _randn(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _u32(t):
    return np.ascontiguousarray(_np(t)).view(np.uint32)


def _assert_bits(got, want, what=""):
    """float32 arrays equal as int32 bit patterns; a NaN equals any NaN."""
    got, want = np.ascontiguousarray(_np(got), dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.int32)[~gn] == want.view(np.int32)[~wn]).all(), what


def _center(D, seed):
    return (0.5 * _randn((D,), seed) / float(np.sqrt(D))).contiguous()


_models = {}


def _model(D):
    """Seeded rows, queries and a centre of one dim with the model's codes, weighted distances and scores, once per dim."""
    if D not in _models:
        x, q, c = _randn((GMAX, D), 100 + D), _randn((NQ, D), 200 + D), _center(D, 300 + D)
        codes = R.encode(_np(M.l2_normalize_rows(x)), _np(c))
        m, s, u, l1, nan = A.model(_np(M.l2_normalize_rows(q)), codes, _np(c))
        assert not nan.any()
        _models[D] = dict(x=x, q=q, c=c, codes=codes, m=m, s=s, u=u, l1=l1, gal={})
    return _models[D]


def _gallery(m, D, G):
    if G not in m["gal"]:
        m["gal"][G] = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][:G])
    return m["gal"][G]


# ---- 1. the query quantiser
@pytest.mark.parametrize("D", CODE_DIMS)
def test_query_codes_equal_the_model(D):
    q = _randn((70, D), 400 + D)
    q[3] = 0.0                                                       # a zero-norm query
    q[7] = 1e-9 * q[8]                                               # norm below eps
    q[9, D // 2] = float("nan")
    q[11, 0] = float("inf")
    qn = M.l2_normalize_rows(q)
    for c in (None, _center(D, 500 + D), qn[5].clone()):             # the last: query 5 IS the centre, L1 == 0
        bg = binary.BinaryGallery(D, DEV, center=c)
        u, l1, nan = bg.query_codes(q)
        assert u.dtype == torch.int8 and l1.dtype == torch.int32 and nan.dtype == torch.bool
        wu, wl, wn = A.query_codes(_np(qn), None if c is None else _np(c))
        what = f"D={D} centre={'none' if c is None else 'given'}"
        assert (_np(nan) == wn).all(), what
        assert (_np(u) == wu).all(), what
        assert (_np(l1) == wl).all(), what
        assert wn[9] and wn[11] and (wu[[9, 11]] == 0).all()
    assert wl[5] == 0 and not wn[5]                                  # (the last centre)
    wu0, wl0, wn0 = A.query_codes(_np(qn))
    assert wl0[3] == 0 and not wn0[3]                                # the all-zero query with a zero centre
    assert binary.BinaryGallery(D, DEV).query_codes(q[:0])[0].shape == (0, D)


def test_special_queries_score_by_the_rules():
    D = 130
    m = _model(D)
    gal = _gallery(m, D, GMAX)
    raw = m["q"][:6]
    qn = M.l2_normalize_rows(raw)
    q = raw.clone()
    q[1, 7] = float("nan")                                           # a NaN query
    q[2] = 0.0                                                       # an all-zero query: n = 0, r = -centre
    wm, ws, wu, wl, wn = A.model(_np(M.l2_normalize_rows(q)), m["codes"], _np(m["c"]))
    assert wn.tolist() == [False, True, False, False, False, False]
    d = gal.distances(q, asymmetric=True)
    assert (_np(d) == wm).all() and (_np(d)[1] == -1).all()
    for k in (3, 150):
        v, i = gal.search(q, k, idx_offset=50, asymmetric=True)
        wv, wi = R.select(ws, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi + 50).all()
        assert torch.isnan(v[1]).all() and (_np(i[1]) == np.arange(k) + 50).all()
    # L1 == 0: a gallery whose centre is the query's normalised row scores 0.0 against every row, the rows in order
    at = binary.BinaryGallery(D, DEV, center=qn[4].clone()).add(m["x"])
    _, l1, nan = at.query_codes(raw[4:5])
    assert int(l1[0]) == 0 and not bool(nan[0])
    assert (_np(at.distances(raw[4:5], asymmetric=True)) == 0).all()
    for k in (3, 150):
        v, i = at.search(raw[4:5], k, asymmetric=True)
        assert (_np(v).view(np.int32) == 0).all() and (_np(i)[0] == np.arange(k)).all()      # +0.0


# ---- 2. distances
@pytest.mark.parametrize("D", DIMS)
def test_distances_equal_the_model(D):
    m = _model(D)
    for G in SIZES:
        gal = _gallery(m, D, G)
        assert (_u32(gal.codes) == m["codes"][:G]).all()
        for Q in QS:
            d = gal.distances(m["q"][:Q], asymmetric=True)
            assert d.dtype == torch.int32 and (_np(d) == m["m"][:Q, :G]).all(), f"D={D} G={G} Q={Q}"
    u, l1, _ = _gallery(m, D, GMAX).query_codes(m["q"])
    assert (_np(u) == m["u"]).all() and (_np(l1) == m["l1"]).all()


# ---- 3. search
@pytest.mark.parametrize("D", DIMS)
def test_search_equals_the_model(D):
    m = _model(D)
    for G in SIZES:
        gal = _gallery(m, D, G)
        for Q in (QS if G == GMAX else (1, 5, AQB + 1)):
            for k in sorted({min(k, G) for k in KS}):
                v, i = gal.search(m["q"][:Q], k, asymmetric=True)
                path = lib().mi355_rank_last_path()
                what = f"D={D} G={G} Q={Q} k={k}"
                assert path == PATH_ASYM | (FUSED if k <= 8 else BITONIC), what
                wv, wi = R.select(m["s"][:Q, :G], k)
                _assert_bits(v, wv, what)
                assert (_np(i) == wi).all(), what


def test_more_queries_than_one_launch():
    """300 queries: two scan launches of 256, the second starting at a tile that is not the first."""
    D = 96
    m = _model(D)
    gal = _gallery(m, D, GMAX)
    q = _randn((300, D), 31)
    wm, ws, _, _, _ = A.model(_np(M.l2_normalize_rows(q)), m["codes"], _np(m["c"]))
    assert (_np(gal.distances(q, asymmetric=True)) == wm).all()
    for k in (3, 150):
        v, i = gal.search(q, k, asymmetric=True)
        wv, wi = R.select(ws, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all()


def test_a_launch_that_starts_inside_a_query_tile():
    """For k > 8 the queries of one launch are as many as fit 2^26 candidates (8 per chunk and 256 per k / 8): over 8.5M rows
    that is 252, no multiple of the 32-query tile, so the second launch starts at row 28 of a tile whose first 28 rows belong
    to the first launch.  A score depends on the query, the centre and the code row alone, so the call over all queries must
    return, bit for bit, what the two pieces return when each is searched on its own (one launch each, starting at a tile);
    those are the searches the other tests hold against the model.  D = 32: one word per row, 136 MB of codes."""
    D, G, k = 32, 8500000, 9
    cand_ld = -(-G // CHUNK) * 8 + (k // 8) * CHUNK
    fit = (1 << 26) // cand_ld                                      # BIN_CAND_ELEMS / bin_cand_ld (csrc/binary.hip)
    assert fit == 252 and fit % 32 != 0
    g = torch.Generator(device=DEV).manual_seed(5)
    gal = binary.BinaryGallery(D, DEV, center=_center(D, 6), capacity=G)
    for a in range(0, G, 1 << 20):                                   # in blocks: 128 MB of fp32 rows at a time
        gal.add(torch.randn((min(1 << 20, G - a), D), generator=g, device=DEV))
    q = _randn((fit + 48, D), 7)
    q[fit + 3, 0] = float("nan")                                     # a NaN query in the second launch
    ex = torch.arange(fit + 48, device=DEV) * 1000
    for kw in ({}, {"exclude": ex, "idx_offset": 0}):
        v, i = gal.search(q, k, asymmetric=True, **kw)
        assert lib().mi355_rank_last_path() == PATH_ASYM | BITONIC
        for a, b in ((0, fit), (fit, fit + 48)):
            kw_p = {n: (t[a:b] if torch.is_tensor(t) else t) for n, t in kw.items()}
            pv, pi = gal.search(q[a:b], k, asymmetric=True, **kw_p)
            what = f"queries {a}..{b} {sorted(kw)}"
            assert torch.equal(i[a:b], pi), what
            assert torch.equal(v[a:b].view(torch.int32)[~torch.isnan(pv)], pv.view(torch.int32)[~torch.isnan(pv)]), what
            assert torch.equal(torch.isnan(v[a:b]), torch.isnan(pv)), what
    assert torch.isnan(v[fit + 3]).all() and not torch.isnan(v[fit + 2]).any()
    v, i = gal.search(q, k, asymmetric=True)
    d = gal.distances(q[fit - 2: fit + 2], asymmetric=True)         # and the best row's distance is what distances reports
    best = torch.gather(d, 1, i[fit - 2: fit + 2, :1].to(torch.int64))
    assert (best[:, 0] == d.min(dim=1).values).all()


@pytest.mark.parametrize("D", [33, 1536, 2560])
def test_ties_go_to_the_lower_row(D):
    m = _model(D)
    G = 2 * CHUNK + 1
    q = m["q"][:70]
    same = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][:1].expand(G, D).contiguous())
    for k in (1, 8, 9, 150, G):
        v, i = same.search(q, k, asymmetric=True)
        assert lib().mi355_rank_last_path() == PATH_ASYM | (FUSED if k <= 8 else BITONIC)
        assert (_np(i) == np.arange(k)[None, :]).all(), k
        _assert_bits(v, np.repeat(m["s"][:70, :1], k, axis=1), f"k={k}")
    G = 5 * CHUNK + 7                                                # five rows, each repeated across the chunk edges
    rep = torch.arange(G, device=DEV) % 5
    gal = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][rep])
    s = m["s"][:70, _np(rep)]
    assert (_np(gal.distances(q, asymmetric=True)) == m["m"][:70, _np(rep)]).all()
    for k in (3, 8, 150, 1024):
        v, i = gal.search(q, k, asymmetric=True)
        wv, wi = R.select(s, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all(), k
        v2, i2 = gal.search(q, k, idx_offset=10 ** 6, asymmetric=True)
        assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(i2, i + 10 ** 6)


def test_large_k_selects_through_the_saturated_chunks():
    """The construction of test_binary_gpu.py: forty chunks, the copies of two queries packed into one or two of them, every k
    around the slot count k / 8, with and without a filter."""
    D = 96
    m = _model(D)
    G, Q = 40 * CHUNK + 5, 6
    x = _randn((G, D), 77)
    x[100:420] = m["q"][0]                                           # 320 copies of query 0 over the edge of chunks 0 and 1
    x[5000:5012] = m["q"][1]                                         # 12 copies of query 1 inside chunk 19: 8 are reported
    x[G - 3:] = m["q"][2]                                            # and of query 2 in the last, short chunk
    gl = torch.arange(G, device=DEV) % 3
    gal = binary.BinaryGallery(D, DEV, center=m["c"]).add(x, gl)
    q = m["q"][:Q].clone()
    q[5, 1] = float("nan")
    codes = R.encode(_np(M.l2_normalize_rows(x)), _np(m["c"]))
    assert (_u32(gal.codes) == codes).all()
    _, s, _, _, nan = A.model(_np(M.l2_normalize_rows(q)), codes, _np(m["c"]))
    assert nan.tolist() == [False] * 5 + [True]
    ql = torch.arange(Q, device=DEV) % 3
    ex = torch.tensor([100, 5003, -1, 7, 8, 0], device=DEV)
    mask = (_np(gl)[None, :] != _np(ql)[:, None]) & (np.arange(G)[None, :] != _np(ex)[:, None])
    for k in (9, 15, 16, 17, 150, 320, 321, 1024):
        v, i = gal.search(q, k, asymmetric=True)
        assert lib().mi355_rank_last_path() == PATH_ASYM | BITONIC
        wv, wi = R.select(s, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all(), k
        v, i = gal.search(q, k, query_labels=ql, label_filter="different", exclude=ex, asymmetric=True)
        wv, wi = R.select(s, k, mask)
        _assert_bits(v, wv, f"k={k} filtered")
        assert (_np(i) == wi).all(), k
    assert (_np(gal.search(q[:1], 320, asymmetric=True)[1])[0] == np.arange(100, 420)).all()


@pytest.mark.parametrize("D", [96, 1536])
def test_filters_equal_the_models_mask(D):
    m = _model(D)
    G, off = GMAX, 5000
    gl = torch.randint(0, 20, (G,), generator=torch.Generator().manual_seed(D)).to(DEV)
    ql = torch.randint(0, 20, (NQ,), generator=torch.Generator().manual_seed(D + 1)).to(DEV)
    ex = (torch.arange(NQ, device=DEV) * 7 % G) + off
    ex[1] = -1
    gal = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][:G], gl)
    same = _np(gl)[None, :] == _np(ql)[:, None]
    not_ex = (np.arange(G)[None, :] + off) != _np(ex)[:, None]
    for Q in (1, NQ):
        for k in (3, 8, 150):
            for label_filter, mask in (("same", same), ("different", ~same), (None, np.ones_like(same))):
                wv, wi = R.select(m["s"][:Q, :G], k, (mask & not_ex)[:Q])
                wi = np.where(wi >= 0, wi + off, -1)
                v, i = gal.search(m["q"][:Q], k, idx_offset=off, query_labels=ql[:Q], label_filter=label_filter, exclude=ex[:Q],
                                  asymmetric=True)
                what = f"Q={Q} k={k} {label_filter}"
                _assert_bits(v, wv, what)
                assert (_np(i) == wi).all(), what


# ---- 4. the key (m << 8 | row) at the largest distance there is
def test_key_packing_at_the_largest_distance():
    D, G = 65536, 300
    x = _randn((G, D), 41)
    sign = torch.where(_randn((D,), 42) >= 0, 1.0, -1.0)
    q = _randn((3, D), 43)
    q[0] = sign / 256.0                                              # a unit row of +-1/256: u = +-127 everywhere
    x[17] = -q[0]
    x[200] = q[0]
    gal = binary.BinaryGallery(D, DEV).add(x)                        # zero centre
    codes = R.encode(_np(M.l2_normalize_rows(x)))
    assert (_u32(gal.codes) == codes).all()
    wm, ws, wu, wl, wn = A.model(_np(M.l2_normalize_rows(q)), codes)
    assert (np.abs(wu[0]) == 127).all() and wl[0] == 127 * 65536 and wm[0, 17] == 127 * 65536 and wm[0, 200] == 0
    u, l1, nan = gal.query_codes(q)
    assert (_np(u) == wu).all() and (_np(l1) == wl).all() and not _np(nan).any()
    assert (_np(gal.distances(q, asymmetric=True)) == wm).all()
    for k in (1, 8, G):
        v, i = gal.search(q, k, asymmetric=True)
        wv, wi = R.select(ws, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all(), k
        assert float(v[0, 0]) == 1.0 and int(i[0, 0]) == 200
    assert float(v[0, G - 1]) == -1.0 and int(i[0, G - 1]) == 17


# ---- 5. the refined search
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", [96, 1536])
def test_refine_rescoring(D, dtype):
    m = _model(D)
    G = 500
    gal = _gallery(m, D, G)
    exact = Gallery(D, DEV, dtype=dtype).add(m["x"][:G])
    ivf = IVFIndex(exact, M.l2_normalize_rows(m["x"][:1]), torch.zeros(G, dtype=torch.int64, device=DEV))   # one list: every row
    q = m["q"]
    full_v, full_i = ivf.search(q, G, 1)                            # every pair's fp32 dot, in its order
    for k in (3, 150):
        v, i = gal.search(q, k, refine=exact, shortlist=G, asymmetric=True)
        assert torch.equal(v.view(torch.int32), full_v[:, :k].contiguous().view(torch.int32)) and torch.equal(i, full_i[:, :k])
    dots = np.empty((NQ, G), np.float32)
    np.put_along_axis(dots, _np(full_i), _np(full_v), axis=1)
    for k, short in ((3, 8), (3, 20), (8, 100), (20, 150)):
        _, si = R.select(m["s"][:, :G], short)                      # the model's shortlist = the plain asymmetric search's
        assert (_np(gal.search(q, short, asymmetric=True)[1]) == si).all()
        mask = np.zeros((NQ, G), bool)
        np.put_along_axis(mask, si, True, axis=1)
        wv, wi = R.select(dots, k, mask)
        v, i = gal.search(q, k, refine=exact, shortlist=short, asymmetric=True)
        _assert_bits(v, wv, f"k={k} shortlist={short}")
        assert (_np(i) == wi).all()
    v, i = gal.search(q, 3, refine=exact, asymmetric=True)           # the default shortlist: min(max(10 k, 100), 1024, rows)
    v2, i2 = gal.search(q, 3, refine=exact, shortlist=100, asymmetric=True)
    assert torch.equal(i, i2) and torch.equal(v.view(torch.int32), v2.view(torch.int32))


# ---- 6. the recall condition, on the GPU's own codes
@pytest.mark.parametrize("pooled", [False, True], ids=["raw", "pooled"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_recall_condition_on_gpu_codes(seed, pooled):
    """The condition of tests/test_binary_asym_ref.py evaluated on what the GPU made: its gallery codes, its query codes and
    its weighted distances are the model's bits, so the numbers are the model's exactly."""
    x64, q64 = R.planted_mixture(seed)
    if pooled:
        x64, q64 = R.pooled(x64), R.pooled(q64)
    x, q = torch.from_numpy(x64.astype(np.float32)).to(DEV), torch.from_numpy(q64.astype(np.float32)).to(DEV)
    n, qn = _np(M.l2_normalize_rows(x)), _np(M.l2_normalize_rows(q))
    D = x.shape[1]
    bg = binary.BinaryGallery(D, DEV).train(x).add(x)
    c = _np(bg.center)
    want_g = R.encode(n, c)
    assert (_u32(bg.codes) == want_g).all()
    wm, ws, wu, wl, wn = A.model(qn, want_g, c)
    u, l1, nan = bg.query_codes(q)
    assert (_np(u) == wu).all() and (_np(l1) == wl).all() and (_np(nan) == wn).all()
    gm = _np(bg.distances(q, asymmetric=True))
    assert (gm == wm).all()
    sym = R.scores(_np(bg.distances(q)), D)
    asym = A.scores(gm, _np(l1))
    got = {short: (A.refined_recall(n, qn, sym, 10, short), A.refined_recall(n, qn, asym, 10, short)) for short in (30, 100)}
    assert got[30][1] == A.refined_recall(n, qn, ws, 10, 30) and got[100][1] == A.refined_recall(n, qn, ws, 10, 100)
    print(f"seed {seed} {'pooled' if pooled else 'raw'}: refined recall@10 symmetric / asymmetric at 30: {got[30][0]:.4f} / "
          f"{got[30][1]:.4f}, at 100: {got[100][0]:.4f} / {got[100][1]:.4f}")
    assert got[30][1] >= got[30][0] + 0.05
    assert got[100][0] >= 0.95 and got[100][1] >= 0.95
    # The library's own refined search against that number.  It ranks by fp32 dots where the model ranks by float64 cosines:
    # they can part only where two rows lie within an fp32 rounding (1e-7) of each other at the cut of a shortlist or of the
    # top 10, and the neighbours of a row of this mixture are about 1e-3 apart - so at most a slot or two of the 640.
    exact = Gallery(D, DEV).add(x)
    mean, _ = bg.recall(q, 10, exact, asymmetric=True, refine=exact, shortlist=30)
    print(f"seed {seed}: BinaryGallery.recall(asymmetric=True, refine=, shortlist=30): {mean:.4f}")
    assert abs(mean - got[30][1]) <= 2.0 / 640.0
    assert mean >= got[30][0] + 0.05 - 2.0 / 640.0


# ---- 7. the default is what it was
def test_asymmetric_false_is_the_call_without_it():
    D = 1536
    m = _model(D)
    gal = _gallery(m, D, GMAX)
    exact = Gallery(D, DEV).add(m["x"])
    q = m["q"]
    assert torch.equal(gal.distances(q), gal.distances(q, asymmetric=False))
    assert not torch.equal(gal.distances(q), gal.distances(q, asymmetric=True))
    for kw in ({"k": 3}, {"k": 150}, {"k": 5, "refine": exact, "shortlist": 40}, {"k": 8, "idx_offset": 9, "exclude": torch.arange(NQ, device=DEV)}):
        v, i = gal.search(q, **kw)
        assert lib().mi355_rank_last_path() & 0xff == 10
        v2, i2 = gal.search(q, asymmetric=False, **kw)
        assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(i, i2)
    qc = R.encode(_np(M.l2_normalize_rows(q)), _np(m["c"]))
    wv, wi = R.select(R.scores(R.distances(qc, m["codes"]), D), 150)
    v, i = gal.search(q, 150)
    _assert_bits(v, wv)
    assert (_np(i) == wi).all()


# ---- 8. side streams
SD = 130


def _stream_gallery():
    x = _randn((600, SD), 902)
    return binary.BinaryGallery(SD, DEV, center=_center(SD, 901)).add(x, torch.arange(600, device=DEV) % 7), x


def _pair(shape):
    return {"x": _randn(shape, 903)}, {"x": _randn(shape, 904)}


def _make_search(dev):
    g, _ = _stream_gallery()
    ql = torch.arange(37, device=dev) % 7
    return (lambda i: (g.search(i["x"], 3, asymmetric=True), g.search(i["x"], 150, asymmetric=True),
                       g.search(i["x"], 8, query_labels=ql, label_filter="different", asymmetric=True)),) + _pair((37, SD))


def _make_refined(dev):
    g, x = _stream_gallery()
    f32, f16 = Gallery(SD, dev).add(x), Gallery(SD, dev, dtype=torch.float16).add(x)
    return (lambda i: (g.search(i["x"], 5, refine=f32, asymmetric=True),
                       g.search(i["x"], 5, refine=f16, shortlist=64, asymmetric=True)),) + _pair((37, SD))


def _make_distances(dev):
    g, _ = _stream_gallery()
    return (lambda i: g.distances(i["x"], asymmetric=True),) + _pair((37, SD))


def _make_query_codes(dev):
    g, _ = _stream_gallery()
    return (lambda i: g.query_codes(i["x"]),) + _pair((37, SD))


STREAM_CASES = [H.Case("BinaryGallery.search asymmetric", ("BinaryGallery.search",), _make_search, syncs=False),
                H.Case("BinaryGallery.search asymmetric refined", ("BinaryGallery.search",), _make_refined, syncs=False),
                H.Case("BinaryGallery.distances asymmetric", ("BinaryGallery.distances",), _make_distances, syncs=False),
                H.Case("BinaryGallery.query_codes", ("BinaryGallery.query_codes",), _make_query_codes, syncs=False)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
