"""fp4 resident gallery on the GPU: the conversion, every search path, the filters and the range search against the NumPy model
of the contract (gallery_fp4_ref.py) BIT FOR BIT - every partial sum of a dot product is a multiple of 0.25 that fp32 holds
exactly, so there is no tolerance and no tie slack anywhere - plus the properties the other galleries are tested for (a score
depends on its query and row only).  The saturated rows are the probe of that exactness on the scaled fp4 MFMA."""
import ctypes

import numpy as np
import pytest
import torch

import gallery_fp4_ref as R
import imageretrievalresearch_amd as M
import stream_harness as H
from imageretrievalresearch_amd import Gallery, Int8Gallery, MI355Error
from imageretrievalresearch_amd._lib import lib
from imageretrievalresearch_amd.fp4 import FP4Gallery

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_FP4_GEMM, PATH_FP4_GEMV, FUSED, BITONIC = 12, 13, 0x100, 0x200
NQ = 200                                                            # queries of every model; each Q of a test is a prefix


def _randn(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _assert_bits(got, want, what=""):
    """float32 arrays equal as int32 bit patterns; a NaN equals any NaN."""
    got, want = np.ascontiguousarray(_np(got) if torch.is_tensor(got) else got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.int32)[~gn] == want.view(np.int32)[~wn]).all(), what


def _model_of(x, q, gl=None):
    """The FP4Gallery of the rows x, and the model's scores and full order of the queries q against them."""
    D = x.shape[1]
    gal = FP4Gallery(D, DEV).add(x, gl)
    codes, mult = R.quantize_rows(_np(M.l2_normalize_rows(x)))
    hi, lo, s_q = R.query_planes(_np(M.l2_normalize_rows(q)))
    s = R.scores(hi, lo, s_q, codes, mult)
    assert (_np(gal.codes) == R.pack(codes)[:, : (D + 1) // 2]).all()
    _assert_bits(gal.mults, mult, "mults")
    return dict(x=x, q=q, gal=gal, s=s, top=R.topk(s, min(1024, x.shape[0])), gl=gl, codes=codes)


_models = {}


def _model(D, G, labels=False):
    """A seeded gallery of G rows and NQ queries, once per (D, G)."""
    key = (D, G, labels)
    if key not in _models:
        gl = torch.randint(0, 50, (G,), generator=torch.Generator().manual_seed(D + G)).to(DEV) if labels else None
        _models[key] = _model_of(_randn((G, D), 100 + D + G), _randn((NQ, D), 200 + D + G), gl)
    return _models[key]


# ---- 1. conversion
@pytest.mark.parametrize("D", [1, 2, 255, 256, 257, 1536])
def test_conversion_bit_for_bit(D):
    x = _randn((1000, D), D)
    x[3] = 0.0
    x[10, D // 2] = float("nan")
    x[20] = 0.0
    x[20, D - 1] = -2.5                                              # one non-zero element
    x[30] = 0.37 * torch.where(torch.arange(D, device=DEV) % 3 == 0, -1.0, 1.0)   # equal magnitudes: every code +-6
    x[40] = 1e-9 * x[41]                                             # norm below eps
    ties = torch.tensor(np.concatenate([R.TIES, -R.TIES, [6.0]]), dtype=torch.float32, device=DEV)
    for r, s in ((50, 1.0), (51, 0.125), (52, 3.0)):                 # within a rounding of every tie once normalised
        x[r] = ties[torch.arange(D, device=DEV) % len(ties)] * s
        x[r, 0] = 6.0 * s
    gal = FP4Gallery(D, DEV, capacity=1)
    cap0 = gal._codes.shape[0]
    for a, b in ((0, 1), (1, 300), (300, 301), (301, 1000)):
        gal.add(x[a:b])
    assert len(gal) == 1000 and gal._codes.shape[0] > cap0           # the buffers grew with a resident row in them
    codes, mults = R.quantize_rows(_np(M.l2_normalize_rows(x)))
    assert np.isnan(mults[10]) and mults[3] == 0 and (np.abs(R.twice(codes[30])) == 12).all() and np.abs(R.twice(codes[40])).max() == 12
    ld = R.stride(D)
    nb = (D + 1) // 2
    assert gal.codes.shape == (1000, nb) and gal.codes.dtype == torch.uint8 and gal.mults.shape == (1000,)
    assert (_np(gal.codes) == R.pack(codes)[:, :nb]).all()
    _assert_bits(gal.mults, mults)
    assert gal._codes.shape[1] == ld and (_np(gal._codes[:1000]) == R.pack(codes)).all()    # the padding nibbles are zero
    assert gal.nbytes == gal._codes.shape[0] * (ld + 4)
    assert lib().mi355_gallery_fp4_bytes(1000, D) == 1000 * ld
    live = ~np.isnan(mults)
    deq = gal.dequantized()
    assert deq.shape == (1000, D) and deq.dtype == torch.float32
    assert torch.equal(deq[torch.from_numpy(live).to(DEV)], torch.from_numpy(R.value(codes[live]) * mults[live, None]).to(DEV))


def test_exact_ties_go_to_the_even_neighbour():
    """Rows taken as they are (the path of from_gallery) with amax = 6 * 2^e: a_i = n_i exactly, every tie is exact."""
    ties = np.concatenate([R.TIES, -R.TIES, R.MAGNITUDES, [6.0, -6.0, 0.2, -0.2, 5.5]]).astype(np.float32)
    n = np.stack([ties * np.float32(s) for s in (1.0, 0.125, 64.0)])
    gal = FP4Gallery(len(ties), DEV)._append(torch.from_numpy(n).to(DEV), None, normalized=True)
    codes, mults = R.quantize_rows(n)
    assert (R.value(codes[0, :14]) == np.array([0, 1, 1, 2, 2, 4, 4, 0, -1, -1, -2, -2, -4, -4], np.float32)).all()
    assert (codes[1] == codes[0]).all() and (codes[2] == codes[0]).all() and (codes[0, 7] == 0)     # -0.25 -> 0, not -0
    assert (R.unpack(_np(gal.codes), len(ties)) == codes).all()
    _assert_bits(gal.mults, mults)


# ---- 2. every search path equals the model
@pytest.mark.parametrize("G", [1, 127, 129, 1000, 5000])
@pytest.mark.parametrize("D", [1, 255, 256, 257, 600, 1000, 1536])   # 1, 1, 1, 2, 3, 4, 6 k-steps: the gallery ring is 3 deep
def test_search_equals_the_model(D, G):
    m = _model(D, G)
    for Q in (1, 4, 5, 70):
        for k in (3, 150):
            if k > G:
                k = G
            v, i = m["gal"].search(m["q"][:Q], k)
            path = lib().mi355_rank_last_path()
            what = f"D={D} G={G} Q={Q} k={k}"
            _assert_bits(v, m["top"][0][:Q, :k], what)
            assert (_np(i) == m["top"][1][:Q, :k]).all(), what
            if Q <= 4:
                assert path & 0xff == PATH_FP4_GEMV, what
            else:
                assert path == PATH_FP4_GEMM | (FUSED if k <= 8 else BITONIC), what


# ---- 3. saturated rows: the probe of exact accumulation
def _saturated(D, rows, seed):
    """rows float32 rows of +-1 with a trailing run of +-1/12 (codes +-6, then +-0.5); the first half of the rows all positive
    (the sums reach 36 D), the rest with random signs.  Odd rows hold 5/6 where even rows hold 1, but for their first element:
    as queries their hi plane is a tie (4 or 6) and their lo plane +-4."""
    g = torch.Generator().manual_seed(seed)
    x = torch.ones((rows, D))
    x[1::2] = 5.0 / 6.0
    x[:, 0] = 1.0
    for r in range(rows):
        x[r, D - 1 - 3 * r:] = 1.0 / 12.0
    sign = torch.where(torch.rand((rows - rows // 2, D), generator=g) < 0.5, -1.0, 1.0)
    x[rows // 2:] *= sign
    return x.to(DEV)


@pytest.mark.parametrize("D", [4096, 65536])
def test_saturated_rows_are_summed_exactly(D):
    G = 130
    m = _model_of(_saturated(D, G, D), _saturated(D, 8, D + 1))
    t = np.abs(R.twice(m["codes"]))
    assert (t[0::2, : D - 400] == 12).all() and (t[:, -1] == 1).all()                # +-6, then the run of +-0.5
    hi, lo, _ = R.query_planes(_np(M.l2_normalize_rows(m["q"])))
    assert (np.abs(R.twice(hi[0::2, : D - 30])) == 12).all() and (np.abs(R.twice(lo[1::2, 1: D - 30])) == 8).all()
    acc = (R.twice(hi[0]).astype(np.float64) @ R.twice(m["codes"][0]).astype(np.float64)) / 4
    assert acc > 35.9 * D                                             # the all-positive pair: as large as a sum gets
    for Q, k, gemv in ((1, 130, True), (4, 3, D == 4096), (4, 130, D == 4096), (5, 3, False), (8, 130, False)):
        v, i = m["gal"].search(m["q"][:Q], k)
        path = lib().mi355_rank_last_path()
        what = f"D={D} Q={Q} k={k}"
        assert (path & 0xff) == (PATH_FP4_GEMV if gemv else PATH_FP4_GEMM), what    # (4 queries of 32 KB do not fit the GEMV's LDS)
        _assert_bits(v, m["top"][0][:Q, :k], what)
        assert (_np(i) == m["top"][1][:Q, :k]).all(), what


# ---- 4. the seam between the two launches
@pytest.mark.parametrize("k", [3, 150])
def test_tail_launch_is_bit_identical(k):
    """Q = 200 x G = 5000 is 2 x 40 tiles: 8 slots cut them into whole rounds (one launch), 12 slots leave a tail launch.
    D = 600, 1000: three and four k-steps."""
    out = (ctypes.c_int * 5)()
    for D in (600, 1000):
        m = _model(D, 5000)
        want_v, want_i = m["gal"].search(m["q"], k)
        try:
            for slots, tail in ((8, False), (12, True)):
                assert lib().mi355_rank_set_round_slots(slots) == 0
                v, i = m["gal"].search(m["q"], k)
                assert lib().mi355_rank_last_tiles(out, 5) == 5
                assert out[0] == slots and (out[3] > 0) == tail, list(out)
                assert torch.equal(v.view(torch.int32), want_v.view(torch.int32)) and torch.equal(i, want_i), D
        finally:
            assert lib().mi355_rank_set_round_slots(0) == 0
        _assert_bits(want_v, m["top"][0][:, :k], f"D={D}")
        assert (_np(want_i) == m["top"][1][:, :k]).all(), D


# ---- 5. a score depends on its query and its row only
@pytest.mark.parametrize("k", [3, 150])
def test_scores_do_not_depend_on_the_batch(k):
    m = _model(1536, 5000)
    gal, q = m["gal"], m["q"]
    v, i = gal.search(q, k)                                          # Q = 200
    for a, b in ((0, 1), (0, 4), (3, 8), (0, 5), (60, 200)):
        pv, pi = gal.search(q[a:b], k)
        assert torch.equal(pv.view(torch.int32), v[a:b].view(torch.int32)) and torch.equal(pi, i[a:b]), (a, b)
    ov, oi = gal.search(q, k, idx_offset=1000)
    assert torch.equal(ov.view(torch.int32), v.view(torch.int32)) and torch.equal(oi, i + 1000)
    ev, ei = gal.search(q[:0], 5)
    assert ev.shape == (0, 5) and ei.shape == (0, 5)


# ---- 6. ties and NaN
@pytest.mark.parametrize("Q", [1, 64])
def test_duplicates_ascend_and_nan_ranks_first(Q):
    D, G = 1536, 3000
    x = _randn((G, D), 5)
    for r in (17, 40, 2999):
        x[r] = x[5]
    x[7] = float("nan")
    q = x[5:6].repeat(Q, 1) + 1e-3 * _randn((Q, D), 9)
    q[0] = x[5]
    gal = FP4Gallery(D, DEV).add(x)
    v, i = gal.search(q, 8)
    assert torch.isnan(v[:, 0]).all() and (i[:, 0] == 7).all()
    assert i[0, 1:5].tolist() == [5, 17, 40, 2999]                   # equal scores: ascending index
    assert torch.equal(v[0, 1:5].view(torch.int32), v[0, 1:2].view(torch.int32).expand(4))
    q[-1, 3] = float("nan")                                          # a NaN query scores NaN everywhere: the lowest rows first
    v, i = gal.search(q, 4)
    assert torch.isnan(v[-1]).all() and i[-1].tolist() == [0, 1, 2, 3]


# ---- 7. filters
def _eligible(m, Q, ql, label_filter, exclude):
    G = m["s"].shape[1]
    ok = np.ones((Q, G), bool)
    if label_filter is not None:
        same = _np(ql)[:, None] == _np(m["gl"])[None, :]
        ok &= same if label_filter == "same" else ~same
    if exclude is not None:
        ex = _np(exclude)
        ok[np.arange(Q)[ex >= 0], ex[ex >= 0]] = False
    return ok


@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("Q", [3, 70])
def test_filtered_search_equals_the_model(Q, k):
    m = _model(600, 3000, labels=True)
    gal, q = m["gal"], m["q"][:Q]
    gen = torch.Generator().manual_seed(Q * 100 + k)
    ql = torch.randint(0, 50, (Q,), generator=gen).to(DEV)
    ql[1] = 999                                                      # no row has this label: "same" leaves only pads
    ex = torch.randint(-5, 3000, (Q,), generator=gen).to(DEV)
    padded = False
    for lf, e in (("same", None), ("different", None), (None, ex), ("same", ex), ("different", ex)):
        v, i = gal.search(q, k, query_labels=ql if lf else None, label_filter=lf, exclude=e)
        ok = _eligible(m, Q, ql, lf, e)
        wv, wi = R.topk(m["s"][:Q], k, mask=ok)
        _assert_bits(v, wv, (lf, e is not None))
        assert (_np(i) == wi).all(), (lf, e is not None)
        padded = padded or (wi == -1).any()
    assert padded
    with pytest.raises(MI355Error, match="needs gallery labels"):
        FP4Gallery(600, DEV).add(m["x"][:100]).search(q, k, query_labels=ql, label_filter="same")


# ---- 8. range search
@pytest.mark.parametrize("Q", [3, 70])
def test_range_search_equals_the_model(Q):
    m = _model(600, 3000, labels=True)
    gal, q, s = m["gal"], m["q"][:Q], m["s"][:Q]
    keep = max(1, s.size // 100)
    thr_some = float(np.partition(s.ravel(), s.size - keep)[s.size - keep])      # a score itself: >= keeps it
    ql = torch.randint(0, 50, (Q,), generator=torch.Generator().manual_seed(Q)).to(DEV)
    ex = torch.arange(Q, device=DEV) * 7
    for thr, kw, ok in ((thr_some, {}, np.ones(s.shape, bool)),
                        (float(s.max()) + 1e-3, {}, np.ones(s.shape, bool)),
                        (thr_some, dict(query_labels=ql, label_filter="different", exclude=ex), _eligible(m, Q, ql, "different", ex))):
        res = gal.range_search(q, thr, **kw)
        hit = ok & (s.astype(np.float64) >= thr)
        rows, cols = np.nonzero(hit)                                 # row-major: queries in order, rows ascending
        off = np.concatenate([[0], np.cumsum(hit.sum(axis=1))])
        assert (_np(res.offsets) == off).all() and res.offsets.dtype == torch.int64
        assert (_np(res.indices) == cols).all() and res.indices.dtype == torch.int64
        _assert_bits(res.scores, s[rows, cols])
    assert int(gal.range_search(q, thr_some).offsets[-1]) >= keep
    want = Gallery(600, DEV).add(m["x"]).range_search(q, 2.0)        # the layout of Gallery.range_search's result
    got = gal.range_search(q, 2.0)
    assert type(got) is type(want) and [t.shape for t in got] == [t.shape for t in want]


# ---- 9. from_gallery, refine= and recall on the planted mixture
def test_refined_search_and_recall_on_the_planted_mixture():
    x, q = (torch.from_numpy(a).to(DEV) for a in R.mixture())
    lab = torch.arange(R.MIX_G, device=DEV) % 97
    exact = Gallery(R.MIX_D, DEV).add(x, lab)
    gal, added = FP4Gallery.from_gallery(exact), FP4Gallery(R.MIX_D, DEV).add(x, lab)
    assert isinstance(gal, FP4Gallery) and len(gal) == R.MIX_G
    assert torch.equal(gal.codes, added.codes) and torch.equal(gal.mults.view(torch.int32), added.mults.view(torch.int32))
    assert torch.equal(gal.labels, lab) and gal.labels.data_ptr() != exact.labels.data_ptr()
    m = R.mixture_recall(_np(exact.data), _np(M.l2_normalize_rows(q)))
    print(f"fp4 model on the library's normalised rows: raw recall@10 {m['raw']:.4f}, refined at a shortlist of 30 {m['refined']:.4f}")
    v, i = gal.search(q, R.MIX_SHORTLIST)                            # the library returns the model's shortlist ...
    _assert_bits(v, m["vals"])
    assert (_np(i) == m["idx"]).all()
    raw, per = gal.recall(q, R.MIX_K, exact)                         # ... so its recall is the model's
    refined, _ = gal.recall(q, R.MIX_K, exact, refine=exact, shortlist=R.MIX_SHORTLIST)
    print(f"FP4Gallery.recall: raw recall@10 {raw:.4f}, refined at a shortlist of 30 {refined:.4f}")
    assert per.shape == (R.MIX_Q,) and per.dtype == torch.float64
    assert raw >= 0.85
    assert refined == 1.0
    rv, ri = gal.search(q, R.MIX_K, refine=exact, shortlist=R.MIX_SHORTLIST)
    ev, ei = exact.search(q, R.MIX_K)
    assert torch.equal(ri.sort(dim=1).values, ei.sort(dim=1).values) and (rv - ev).abs().max() < 1e-5   # the fp32 rows' scores
    f16 = Gallery(R.MIX_D, DEV, dtype=torch.float16).add(x)
    assert gal.search(q[:7], 5, refine=f16)[1].shape == (7, 5)
    with pytest.raises(MI355Error, match="embedding dims differ"):
        gal.search(q[:, :64], 3)
    with pytest.raises(MI355Error, match="selected index k out of range"):
        FP4Gallery(R.MIX_D, DEV).add(x[:5]).search(q, 6)
    with pytest.raises(MI355Error, match="gallery rows must be"):
        gal.add(x[:, :64])
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        gal.search(q, 3, refine=Int8Gallery(R.MIX_D, DEV))
    with pytest.raises(MI355Error, match="refine must be a Gallery"):
        Int8Gallery(R.MIX_D, DEV).add(x[:50]).search(q, 3, refine=FP4Gallery(R.MIX_D, DEV).add(x[:50]))


def test_queries_on_another_device_are_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    gal = FP4Gallery(16, DEV).add(_randn((10, 16), 1))
    with pytest.raises(MI355Error, match="queries on"):
        gal.search(torch.zeros(2, 16, device="cuda:1"), 1)
    with pytest.raises(MI355Error, match="queries on"):
        gal.range_search(torch.zeros(2, 16, device="cuda:1"), 0.5)


# ---- 10. side streams
SD = 300


def _stream_gallery():
    x = _randn((600, SD), 902)
    return FP4Gallery(SD, DEV).add(x, torch.arange(600, device=DEV) % 7), x


def _pair(shape):
    return {"x": _randn(shape, 903)}, {"x": _randn(shape, 904)}


def _make_add(dev):
    def op(i):
        g = FP4Gallery(SD, dev, capacity=1).add(i["x"][:100]).add(i["x"][100:])       # grows with rows resident
        return g.codes, g.mults, g.dequantized(), g.nbytes
    return (op,) + _pair((3000, SD))


def _make_from_gallery(dev):
    def op(i):
        g = FP4Gallery.from_gallery(Gallery(SD, dev).add(i["x"]))
        return g.codes, g.mults
    return (op,) + _pair((3000, SD))


def _make_search(dev):
    g, _ = _stream_gallery()
    ql = torch.arange(37, device=dev) % 7
    return (lambda i: (g.search(i["x"], 3), g.search(i["x"], 150), g.search(i["x"][:2], 3),
                       g.search(i["x"], 8, query_labels=ql, label_filter="different")),) + _pair((37, SD))


def _make_refined(dev):
    g, x = _stream_gallery()
    f32, f16 = Gallery(SD, dev).add(x), Gallery(SD, dev, dtype=torch.float16).add(x)
    return (lambda i: (g.search(i["x"], 5, refine=f32), g.search(i["x"], 5, refine=f16, shortlist=64)),) + _pair((37, SD))


def _make_range(dev):
    g, _ = _stream_gallery()
    return (lambda i: g.range_search(i["x"], 0.1),) + _pair((37, SD))


def _make_recall(dev):
    g, x = _stream_gallery()
    exact = Gallery(SD, dev).add(x)
    return (lambda i: g.recall(i["x"], 10, exact),) + _pair((37, SD))


STREAM_CASES = [H.Case("FP4Gallery.add", ("FP4Gallery.add",), _make_add, syncs=False),
                H.Case("FP4Gallery.from_gallery", ("FP4Gallery.from_gallery",), _make_from_gallery, syncs=False),
                H.Case("FP4Gallery.search", ("FP4Gallery.search",), _make_search, syncs=False),
                H.Case("FP4Gallery.search refined", ("FP4Gallery.search",), _make_refined, syncs=False),
                H.Case("FP4Gallery.range_search", ("FP4Gallery.range_search",), _make_range, syncs=True),   # each block's hit count
                H.Case("FP4Gallery.recall", ("FP4Gallery.recall",), _make_recall, syncs=True)]              # returns a float


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
