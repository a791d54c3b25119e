"""Binary (sign-bit) resident gallery on the GPU: the encoder, the distances, every search path, the filters, the refined
search, training and the side-stream behaviour against the NumPy model of the contract (binary_ref.py) BIT FOR BIT - the
arithmetic is integer but for one fp32 division, so there is no tolerance and no tie slack anywhere."""
import numpy as np
import pytest
import torch

import binary_ref as R
import imageretrievalresearch_amd as M
import stream_harness as H
from imageretrievalresearch_amd import Gallery, IVFIndex, MI355Error, binary
from imageretrievalresearch_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_BINARY, FUSED, BITONIC = 10, 0x100, 0x200
CHUNK, B = binary.SCAN_CHUNK, binary.QUERY_BLOCK
# one, two, two (a full word) and two words in a stored row of four; three words and one pad word; four words, none; five words
# stored as eight (a 16-word slice); 32 and 48 words (a whole 48-word slice, the second with no pad); 80 words = two slices
DIMS = [1, 31, 32, 33, 96, 128, 130, 1000, 1536, 2560]
SIZES = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
GMAX = 2 * CHUNK + 1                                                # rows of every model; each G of a test is a prefix
P = binary.SELECT_PASS                                              # queries of one pass of the in-kernel selection
QS = [1, 4, 5, P - 1, P, P + 1, B - 1, B, B + 1]
NQ = B + 1                                                          # queries of every model; each Q of a test is a prefix
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
    """A centre at the scale of a unit row's elements, so that it decides a fair share of the bits."""
    return (0.5 * _randn((D,), seed) / float(np.sqrt(D))).contiguous()


_models = {}


def _model(D):
    """Seeded rows, queries and a centre of one dim with the model's codes, distances and scores, once per dim."""
    if D not in _models:
        x, q, c = _randn((GMAX, D), 100 + D), _randn((NQ, D), 200 + D), _center(D, 300 + D)
        codes = R.encode(_np(M.l2_normalize_rows(x)), _np(c))
        qcodes = R.encode(_np(M.l2_normalize_rows(q)), _np(c))
        d = R.distances(qcodes, codes)
        _models[D] = dict(x=x, q=q, c=c, codes=codes, d=d, s=R.scores(d, D), gal={})
    return _models[D]


def _gallery(m, D, G):
    """The BinaryGallery of the model's first G rows."""
    if G not in m["gal"]:
        m["gal"][G] = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][:G])
    return m["gal"][G]


# ---- 1. encode and append
@pytest.mark.parametrize("D", DIMS)
def test_encode_bit_for_bit(D):
    x = _randn((300, D), D)
    x[3] = 0.0                                                       # a zero-norm row
    x[10, D // 2] = float("nan")                                     # a NaN: its bit is 0
    x[40] = 1e-9 * x[41]                                             # norm below eps
    x[50, 0] = -0.0
    x[51, D - 1] = 0.0
    x[60, 0] = float("inf")
    n = M.l2_normalize_rows(x)
    at = n[5].clone()                                                # as a centre: row 5 is AT it in every element
    W, ld = binary.words(D), binary.row_words(D)
    for c in (None, _center(D, 7 + D), at):
        gal = binary.BinaryGallery(D, DEV, center=c, capacity=1)
        cap0 = gal._codes.shape[0]
        for a, b in ((0, 1), (1, 100), (100, 101), (101, 300)):
            gal.add(x[a:b])
        assert len(gal) == 300 and gal._codes.shape[0] > cap0        # the buffer grew with a resident row in it
        want = R.encode(_np(n), None if c is None else _np(c))
        assert gal.codes.shape == (300, W) and gal.codes.dtype == torch.int32
        assert (_u32(gal.codes) == want).all()
        assert (_np(gal._codes[:300, W:]) == 0).all()                # pad words
        assert (want[10, (D // 2) // 32] >> np.uint32((D // 2) % 32)) & 1 == 0   # the NaN element: bit 0
        one = binary.BinaryGallery(D, DEV, center=c).add(x)          # one call: the same codes
        assert torch.equal(one.codes, gal.codes)
        assert gal.nbytes == gal._codes.shape[0] * ld * 4 + (0 if c is None else 4 * D)
        # rows taken as they are
        out = torch.full((300, ld), -1, dtype=torch.int32, device=DEV)
        gal._encode(n, True, out)
        assert torch.equal(out, gal._codes[:300])
    full = (1 << (D % 32)) - 1 if D % 32 else 0xffffffff
    assert (want[5, :-1] == 0xffffffff).all() and want[5, -1] == full      # n >= n: every bit of the row, no pad bit
    # +-0 against a zero centre: both reach it
    z = torch.zeros((2, D), device=DEV)
    z[1] = -0.0
    out = torch.empty((2, ld), dtype=torch.int32, device=DEV)
    binary.BinaryGallery(D, DEV)._encode(z, True, out)
    assert (_u32(out[:, :W]) == R.encode(_np(z))).all() and (_u32(out[:, :W])[:, :-1] == 0xffffffff).all()
    with pytest.raises(MI355Error, match=rf"\(n,{D}\)"):
        gal.add(torch.zeros(3, D + 1, device=DEV))
    with pytest.raises(MI355Error, match="queries must be"):
        gal.distances(torch.zeros(3, D + 1, device=DEV))


# ---- 2. distances
@pytest.mark.parametrize("D", DIMS)
def test_distances_equal_the_model(D):
    m = _model(D)
    for G in SIZES:
        gal = _gallery(m, D, G)
        assert (_u32(gal.codes) == m["codes"][:G]).all()
        for Q in QS:
            d = gal.distances(m["q"][:Q])
            assert d.dtype == torch.int32 and (_np(d) == m["d"][:Q, :G]).all(), f"D={D} G={G} Q={Q}"
    nanq = m["q"][:3].clone()
    nanq[1, 0] = float("nan")
    d = _np(_gallery(m, D, GMAX).distances(nanq))
    assert (d[1] == -1).all() and (d[0] == m["d"][0]).all() and (d[2] == m["d"][2]).all()


# ---- 3. search
@pytest.mark.parametrize("D", DIMS)
def test_search_equals_the_model(D):
    m = _model(D)
    for G in SIZES:
        gal = _gallery(m, D, G)
        for Q in (QS if G == GMAX else (1, 5, B + 1)):
            for k in sorted({min(k, G) for k in KS}):
                v, i = gal.search(m["q"][:Q], k)
                path = lib().mi355_rank_last_path()
                what = f"D={D} G={G} Q={Q} k={k}"
                assert path == PATH_BINARY | (FUSED if k <= 8 else BITONIC), what
                wv, wi = R.select(m["s"][:Q, :G], k)
                _assert_bits(v, wv, what)
                assert (_np(i) == wi).all(), what
    # a NaN query: NaN scores, the rows in order; its neighbours are untouched
    gal = _gallery(m, D, GMAX)
    nanq = m["q"][:3].clone()
    nanq[1, 0] = float("nan")
    for k in (3, 150):
        v, i = gal.search(nanq, k, idx_offset=50)
        assert torch.isnan(v[1]).all() and (_np(i[1]) == np.arange(k) + 50).all()
        wv, wi = R.select(m["s"][[0, 2]], k)
        _assert_bits(v[[0, 2]], wv)
        assert (_np(i[[0, 2]]) == wi + 50).all()


@pytest.mark.parametrize("D", [33, 1536, 2560])
def test_ties_go_to_the_lower_row(D):
    m = _model(D)
    G = 2 * CHUNK + 1
    # every row the same: every score tied, the indices ascend from 0
    same = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][:1].expand(G, D).contiguous())
    for k in (1, 8, 9, 150, G):
        v, i = same.search(m["q"], k)
        assert lib().mi355_rank_last_path() == PATH_BINARY | (FUSED if k <= 8 else BITONIC)
        assert (_np(i) == np.arange(k)[None, :]).all(), k
        _assert_bits(v, np.repeat(m["s"][:, :1], k, axis=1), f"k={k}")
    # five rows, each repeated hundreds of times across the chunk edges
    G = 5 * CHUNK + 7
    rep = torch.arange(G, device=DEV) % 5
    gal = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][rep])
    s = m["s"][:, _np(rep)]
    assert (_np(gal.distances(m["q"])) == m["d"][:, _np(rep)]).all()
    for k in (3, 8, 150, 1024):
        v, i = gal.search(m["q"], k)
        wv, wi = R.select(s, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all(), k
        v2, i2 = gal.search(m["q"], k, idx_offset=10 ** 6)
        assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(i2, i + 10 ** 6)


def test_large_k_selects_through_the_saturated_chunks():
    """k > 8 keeps 8 rows per chunk and re-scans the chunks whose 8th row may hide more of the top-k: forty chunks, the best
    rows of two queries packed into one or two of them, every k around the slot count k / 8, with and without a filter."""
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
    qn = _np(M.l2_normalize_rows(q))
    codes = R.encode(_np(M.l2_normalize_rows(x)), _np(m["c"]))
    assert (_u32(gal.codes) == codes).all()
    s = R.scores(R.distances(R.encode(qn, _np(m["c"])), codes, R.has_nan(qn)), D)
    ql = torch.arange(Q, device=DEV) % 3
    ex = torch.tensor([100, 5003, -1, 7, 8, 0], device=DEV)
    mask = (_np(gl)[None, :] != _np(ql)[:, None]) & (np.arange(G)[None, :] != _np(ex)[:, None])
    for k in (9, 15, 16, 17, 150, 320, 321, 1024):
        v, i = gal.search(q, k)
        assert lib().mi355_rank_last_path() == PATH_BINARY | BITONIC
        wv, wi = R.select(s, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all(), k
        v, i = gal.search(q, k, query_labels=ql, label_filter="different", exclude=ex)
        wv, wi = R.select(s, k, mask)
        _assert_bits(v, wv, f"k={k} filtered")
        assert (_np(i) == wi).all(), k
    assert (_np(gal.search(q[:1], 320)[1])[0] == np.arange(100, 420)).all()


# ---- 4. filters
@pytest.mark.parametrize("D", [96, 1536, 2560])
def test_filters_equal_the_models_mask(D):
    m = _model(D)
    G, off = GMAX, 5000
    gl = torch.randint(0, 20, (G,), generator=torch.Generator().manual_seed(D)).to(DEV)
    ql = torch.randint(0, 20, (NQ,), generator=torch.Generator().manual_seed(D + 1)).to(DEV)
    gl[[5, 6, 300]] = 999
    ql[0] = 999                                                      # query 0 has three rows of its label, in two chunks
    ex = (torch.arange(NQ, device=DEV) * 7 % G) + off
    ex[1] = -1
    gal = binary.BinaryGallery(D, DEV, center=m["c"]).add(m["x"][:G], gl)
    s = m["s"][:, :G]
    same = _np(gl)[None, :] == _np(ql)[:, None]
    not_ex = (np.arange(G)[None, :] + off) != _np(ex)[:, None]
    for Q in (1, NQ):
        for k in (3, 8, 150):
            for label_filter, mask in (("same", same), ("different", ~same), (None, np.ones_like(same))):
                wv, wi = R.select(s[:Q], k, (mask & not_ex)[:Q])
                wi = np.where(wi >= 0, wi + off, -1)
                v, i = gal.search(m["q"][:Q], k, idx_offset=off, query_labels=ql[:Q], label_filter=label_filter, exclude=ex[:Q])
                what = f"Q={Q} k={k} {label_filter}"
                _assert_bits(v, wv, what)
                assert (_np(i) == wi).all(), what
    for k in (8, 9):                                                 # fewer eligible rows than k: (-inf, -1) pads, on both paths
        v, i = gal.search(m["q"][:1], k, query_labels=ql[:1], label_filter="same")
        assert sorted(_np(i)[0, :3].tolist()) == [5, 6, 300] and (_np(i)[0, 3:] == -1).all() and torch.isinf(v[0, 3:]).all()
    with pytest.raises(MI355Error):
        binary.BinaryGallery(D, DEV).add(m["x"][:G]).search(m["q"], 3, query_labels=ql, label_filter="same")


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
        v, i = gal.search(q, k, refine=exact, shortlist=G)
        assert torch.equal(v.view(torch.int32), full_v[:, :k].contiguous().view(torch.int32)) and torch.equal(i, full_i[:, :k])
    dots = np.empty((NQ, G), np.float32)
    np.put_along_axis(dots, _np(full_i), _np(full_v), axis=1)
    for k, short in ((3, 8), (3, 20), (8, 100), (20, 150)):
        _, si = R.select(m["s"][:, :G], short)                      # the model's shortlist = the plain binary search's
        assert (_np(gal.search(q, short)[1]) == si).all()
        mask = np.zeros((NQ, G), bool)
        np.put_along_axis(mask, si, True, axis=1)
        wv, wi = R.select(dots, k, mask)
        v, i = gal.search(q, k, refine=exact, shortlist=short)
        _assert_bits(v, wv, f"k={k} shortlist={short}")
        assert (_np(i) == wi).all()
    v, i = gal.search(q, 3, refine=exact)                            # the default shortlist: min(max(10 k, 100), 1024, rows)
    v2, i2 = gal.search(q, 3, refine=exact, shortlist=100)
    assert torch.equal(i, i2) and torch.equal(v.view(torch.int32), v2.view(torch.int32))
    v, i = gal.search(q, 3, idx_offset=700, refine=exact, shortlist=100, exclude=i2[:, 0] + 700)
    elig = np.arange(G)[None, :] != _np(i2[:, :1])                  # the best row left out: of the shortlist, then of the result
    _, si = R.select(m["s"][:, :G], 100, elig)
    mask = np.zeros((NQ, G), bool)
    np.put_along_axis(mask, si, True, axis=1)
    wv, wi = R.select(dots, 3, mask)
    _assert_bits(v, wv, "exclude with an idx_offset")
    assert (_np(i) == wi + 700).all()
    for kw in ({}, {"refine": exact, "shortlist": 50}):
        mean, per = gal.recall(q, 5, exact, **kw)
        got, want = gal.search(q, 5, **kw)[1], exact.search(q, 5)[1]
        share = np.array([len(set(a) & set(b)) / 5.0 for a, b in zip(_np(got).tolist(), _np(want).tolist())])
        # (the device divides by k as a multiplication with 1 / k: the last bit of 3 / 5 may differ from the host's)
        assert np.abs(_np(per) - share).max() <= 1e-15 and mean == pytest.approx(share.mean(), abs=1e-12)


# ---- 6. training
def test_train_sets_the_mean_of_the_moments():
    D = 130
    x = _randn((777, D), 5) + 0.5
    mom = M.embedding_moments(x, normalize=True)
    want = (_np(mom.sum) / float(mom.n)).astype(np.float32)          # the fp32 rounding of the float64 mean
    a, b = binary.BinaryGallery(D, DEV).train(x), binary.BinaryGallery(D, DEV).train(x)
    _assert_bits(a.center, want)
    assert torch.equal(a.center.view(torch.int32), b.center.view(torch.int32))
    close = R.mean_center(_np(M.l2_normalize_rows(x)))               # the same mean in another summation order
    assert np.abs(_np(a.center) - close).max() < 1e-6
    a.add(x)
    with pytest.raises(MI355Error, match="already resident"):
        a.train(x)
    g = Gallery(D, DEV).add(x, torch.arange(777, device=DEV))
    c = binary.BinaryGallery.from_gallery(g)
    assert torch.equal(c.center.view(torch.int32), a.center.view(torch.int32))              # the same rows, the same sums
    assert torch.equal(c.codes, a.codes) and torch.equal(c.labels, g.labels) and len(c) == 777
    with pytest.raises(MI355Error, match="fp16 Gallery"):
        binary.BinaryGallery.from_gallery(Gallery(D, DEV, dtype=torch.float16).add(x))
    with pytest.raises(MI355Error, match=r"center must be \(130,\)"):
        binary.BinaryGallery(D, DEV, center=torch.zeros(D + 1, device=DEV))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_planted_mixture_condition_on_gpu_codes(seed):
    """With the trained centre the refined shortlist finds the float neighbours of pooled (all-positive) rows (>= 0.95);
    with a zero centre it finds nothing (<= 0.10).  The codes are the model's bits, so the numbers are the model's exactly."""
    x64, q64 = R.planted_mixture(seed)
    x, q = torch.from_numpy(R.pooled(x64).astype(np.float32)).to(DEV), torch.from_numpy(R.pooled(q64).astype(np.float32)).to(DEV)
    n, qn = _np(M.l2_normalize_rows(x)), _np(M.l2_normalize_rows(q))
    D = x.shape[1]
    for trained in (True, False):
        bg = binary.BinaryGallery(D, DEV)
        if trained:
            bg.train(x)
        bg.add(x)
        qc = torch.empty((q.shape[0], binary.row_words(D)), dtype=torch.int32, device=DEV)
        bg._encode(q, False, qc)
        c = _np(bg.center) if trained else None
        want_g, want_q = R.encode(n, c), R.encode(qn, c)
        assert (_u32(bg.codes) == want_g).all() and (_u32(qc[:, : bg.W]) == want_q).all()
        got = R.refined_recall(n, qn, _u32(bg.codes), _u32(qc[:, : bg.W]))
        assert got == R.refined_recall(n, qn, want_g, want_q)
        print(f"seed {seed}: {'trained' if trained else 'zero'} centre, refined recall@10 at a shortlist of 100: {got:.4f}")
        assert got >= 0.95 if trained else got <= 0.10
        if trained:                                                  # the library's own refined search agrees with that number
            exact = Gallery(D, DEV).add(x)
            mean, _ = bg.recall(q, 10, exact, refine=exact, shortlist=100)
            print(f"seed {seed}: BinaryGallery.recall(refine=, shortlist=100): {mean:.4f}")
            assert mean >= 0.95


# ---- 7. side streams
SD = 130


def _stream_gallery():
    x = _randn((600, SD), 902)
    return binary.BinaryGallery(SD, DEV, center=_center(SD, 901)).add(x, torch.arange(600, device=DEV) % 7), x


def _pair(shape):
    return {"x": _randn(shape, 903)}, {"x": _randn(shape, 904)}


def _make_add(dev):
    c = _center(SD, 901)

    def op(i):
        g = binary.BinaryGallery(SD, dev, center=c, capacity=1).add(i["x"][:100]).add(i["x"][100:])   # grows with rows resident
        return g.codes
    return (op,) + _pair((3000, SD))


def _make_search(dev):
    g, _ = _stream_gallery()
    ql = torch.arange(37, device=dev) % 7
    return (lambda i: (g.search(i["x"], 3), g.search(i["x"], 150), g.search(i["x"], 8, query_labels=ql, label_filter="different")),) \
        + _pair((37, SD))


def _make_refined(dev):
    g, x = _stream_gallery()
    f32, f16 = Gallery(SD, dev).add(x), Gallery(SD, dev, dtype=torch.float16).add(x)
    return (lambda i: (g.search(i["x"], 5, refine=f32), g.search(i["x"], 5, refine=f16, shortlist=64)),) + _pair((37, SD))


def _make_distances(dev):
    g, _ = _stream_gallery()
    return (lambda i: g.distances(i["x"]),) + _pair((37, SD))


STREAM_CASES = [H.Case("BinaryGallery.add", ("BinaryGallery.add",), _make_add, syncs=False),
                H.Case("BinaryGallery.search", ("BinaryGallery.search",), _make_search, syncs=False),
                H.Case("BinaryGallery.search refined", ("BinaryGallery.search",), _make_refined, syncs=False),
                H.Case("BinaryGallery.distances", ("BinaryGallery.distances",), _make_distances, syncs=False)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
