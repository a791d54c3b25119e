"""Product-quantised resident gallery on the GPU: the encoder, the score slab, every search path, the filters, the centroid
update, the refined search and the side-stream behaviour against the NumPy model of the contract (pq_ref.py) BIT FOR BIT - a
score is a fixed-order sum of table entries, so there is no tolerance and no tie slack anywhere (the one exception is the
update's float64 mean, which the contract lets differ by the summation order: 1 fp32 ulp)."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import pq_ref as R
import stream_harness as H
from imageretrievalresearch_amd import Gallery, IVFIndex, MI355Error, pq
from imageretrievalresearch_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_PQ, FUSED, BITONIC = 9, 0x100, 0x200
NQ = 200                                                            # queries of every model; each Q of a test is a prefix
CHUNK = pq.SCAN_CHUNK
GMAX = CHUNK + 1                                                    # rows of every model; each G of a test is a prefix
# (D, M): dsub 1, 8, 64, 1, 16, then 4 and 4; code loads of 4 bytes (M % 16 != 0) and 16; scan workgroups of 256 threads (M <= 40),
# 512 (M <= 80) and 1024.  The last four: dsub 3, 24, 32 and 33 - no power of two but 32, and k_pq_encode<8>, <32>, <32> (its
# last dsub) and <64> (its first)
SHAPES = [(4, 4), (64, 8), (256, 4), (128, 128), (1536, 96), (192, 48), (176, 44), (12, 4), (96, 4), (128, 4), (132, 4)]
ENCODE_REGS = {3: 8, 24: 32, 32: 32, 33: 64}                        # dsub -> DMAX of the k_pq_encode instance (pq.hip's dispatch)
SIZES = [1, 63, 65, 1000, 2000, CHUNK - 1, CHUNK, CHUNK + 1]


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


def _codebooks(D, Mq, seed):
    """Hand-given random codebooks at the scale of a unit row's sub-vectors."""
    return (_randn((Mq, 256, D // Mq), seed) / float(np.sqrt(D))).contiguous()


_models = {}


def _model(D, Mq):
    """Seeded rows, queries and codebooks of one shape with the model's codes, tables and scores, once per shape."""
    key = (D, Mq)
    if key not in _models:
        x, q, cb = _randn((GMAX, D), 100 + D + Mq), _randn((NQ, D), 200 + D + Mq), _codebooks(D, Mq, 300 + D + Mq)
        codes = R.encode(_np(M.l2_normalize_rows(x)), _np(cb))
        T = R.table(_np(M.l2_normalize_rows(q)), _np(cb))
        _models[key] = dict(x=x, q=q, cb=cb, codes=codes, s=R.scores(T, codes), gal={}, top={})
    return _models[key]


def _gallery(m, D, Mq, G):
    """The PQGallery of the model's first G rows."""
    if G not in m["gal"]:
        m["gal"][G] = pq.PQGallery(D, DEV, Mq, codebooks=m["cb"]).add(m["x"][:G])
    return m["gal"][G]


def _top(m, G):
    if G not in m["top"]:
        m["top"][G] = R.topk(m["s"][:, :G], min(1024, G))
    return m["top"][G]


# ---- 1. encode
@pytest.mark.parametrize("D,Mq", SHAPES)
def test_encode_bit_for_bit(D, Mq):
    dsub = D // Mq
    if dsub in ENCODE_REGS:                                          # the instance this shape is here for
        assert min(r for r in (8, 16, 32, 64) if dsub <= r) == ENCODE_REGS[dsub]
    cb = _codebooks(D, Mq, 7 + D)
    x = _randn((1000, D), D + Mq)
    x[3] = 0.0
    x[10, D // 2] = float("nan")
    x[40] = 1e-9 * x[41]                                             # norm below eps
    gal = pq.PQGallery(D, DEV, Mq, codebooks=cb, capacity=1)
    cap0 = gal._codes.shape[0]
    for a, b in ((0, 1), (1, 300), (300, 301), (301, 1000)):
        gal.add(x[a:b])
    assert len(gal) == 1000 and gal._codes.shape[0] > cap0           # the buffer grew with a resident row in it
    want = R.encode(_np(M.l2_normalize_rows(x)), _np(cb))
    assert gal.codes.shape == (1000, Mq) and gal.codes.dtype == torch.uint8
    assert (_np(gal.codes) == want).all()
    assert want[10, (D // 2) // dsub] == 0                           # the NaN element: code 0 in its subspace
    assert gal.nbytes == gal._codes.shape[0] * Mq + 1024 * D
    # rows taken as they are: a concatenation of centroids returns exactly their codes, a NaN costs its own subspace only
    pick = torch.randint(0, 256, (5, Mq), generator=torch.Generator().manual_seed(D)).to(DEV)
    rows = cb[torch.arange(Mq, device=DEV)[None, :], pick].reshape(5, D).contiguous()
    rows[4, dsub * (Mq - 1)] = float("nan")
    out = torch.empty((5, Mq), dtype=torch.uint8, device=DEV)
    gal._encode(rows, True, out)
    want = _np(pick).astype(np.uint8)
    want[4, Mq - 1] = 0
    assert (_np(out) == want).all()
    assert (_np(out) == R.encode(_np(rows), _np(cb))).all()
    g2 = pq.PQGallery(D, DEV, Mq, codebooks=cb)
    g2._append(rows[:4], None, normalized=True)
    assert torch.equal(g2.reconstruct().view(torch.int32), rows[:4].view(torch.int32))       # the centroids come back


# ---- 2. the score slab
@pytest.mark.parametrize("D,Mq", SHAPES)
def test_scores_equal_the_model(D, Mq):
    m = _model(D, Mq)
    for G in SIZES:
        gal = _gallery(m, D, Mq, G)
        assert (_np(gal.codes) == m["codes"][:G]).all()
        for Q in (1, 5, NQ):
            _assert_bits(gal.scores(m["q"][:Q]), m["s"][:Q, :G], f"D={D} M={Mq} G={G} Q={Q}")
    big = _gallery(m, D, Mq, GMAX)
    one, many = big.scores(m["q"][:1]), big.scores(m["q"])
    assert torch.equal(one.view(torch.int32), many[:1].view(torch.int32))                   # not on Q
    small = _gallery(m, D, Mq, 1000).scores(m["q"])
    assert torch.equal(small.view(torch.int32), many[:, :1000].contiguous().view(torch.int32))   # not on G
    nanq = m["q"][:3].clone()
    nanq[1, 0] = float("nan")
    s = big.scores(nanq)
    assert torch.isnan(s[1]).all() and not torch.isnan(s[0]).any() and not torch.isnan(s[2]).any()


# ---- 3. search
@pytest.mark.parametrize("D,Mq", SHAPES)
def test_search_equals_the_model(D, Mq):
    m = _model(D, Mq)
    for G in (63, 1000, GMAX):
        gal, top = _gallery(m, D, Mq, G), _top(m, G)
        for Q in (1, 5, NQ):
            slab = gal.scores(m["q"][:Q])
            for k in (1, 3, 8, 9, 150, min(1024, G)):
                if k > G:
                    continue
                v, i = gal.search(m["q"][:Q], k)
                path = lib().mi355_rank_last_path()
                what = f"D={D} M={Mq} G={G} Q={Q} k={k}"
                assert path == PATH_PQ | (FUSED if k <= 8 else BITONIC), what
                _assert_bits(v, top[0][:Q, :k], what)
                assert (_np(i) == top[1][:Q, :k]).all(), what
                tv, ti = M.topk(slab, k)
                assert torch.equal(tv.view(torch.int32), v.view(torch.int32)) and torch.equal(ti, i), what


def test_ties_go_to_the_lower_row_and_idx_offset_shifts():
    D, Mq = 64, 8
    m = _model(D, Mq)
    gal = pq.PQGallery(D, DEV, Mq, codebooks=m["cb"]).add(m["x"][:500]).add(m["x"][:500])      # every row twice
    codes = np.concatenate([m["codes"][:500], m["codes"][:500]])
    assert (_np(gal.codes) == codes).all()
    s = np.concatenate([m["s"][:, :500], m["s"][:, :500]], axis=1)
    for k in (8, 150):
        v, i = gal.search(m["q"], k)
        wv, wi = R.topk(s, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all()
        assert torch.equal(v[:, 0::2].view(torch.int32), v[:, 1::2].view(torch.int32))      # the two copies score the same bits
        first, second = _np(i[:, 0::2]), _np(i[:, 1::2])
        assert (first < second).all() and (first % 500 == second % 500).sum() > 0.9 * first.size
        v2, i2 = gal.search(m["q"], k, idx_offset=10 ** 6)
        assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(i2, i + 10 ** 6)


# ---- 4. filters
@pytest.mark.parametrize("D,Mq", [(64, 8), (1536, 96)])
def test_filters_equal_the_models_mask(D, Mq):
    m = _model(D, Mq)
    G, off = 1000, 5000
    gl = torch.randint(0, 50, (G,), generator=torch.Generator().manual_seed(D)).to(DEV)
    ql = torch.randint(0, 50, (NQ,), generator=torch.Generator().manual_seed(D + 1)).to(DEV)
    gl[[5, 6, 7]] = 999
    ql[0] = 999                                                      # query 0 has three rows of its label
    ex = (torch.arange(NQ, device=DEV) * 3 % G) + off
    ex[1] = -1
    gal = pq.PQGallery(D, DEV, Mq, codebooks=m["cb"]).add(m["x"][:G], gl)
    s = m["s"][:, :G]
    same = _np(gl)[None, :] == _np(ql)[:, None]
    not_ex = (np.arange(G)[None, :] + off) != _np(ex)[:, None]
    for Q in (1, NQ):
        for k in (3, 8, 150):
            for label_filter, mask in (("same", same), ("different", ~same), (None, np.ones_like(same))):
                wv, wi = R.topk(s[:Q], k, (mask & not_ex)[:Q])
                wi = np.where(wi >= 0, wi + off, -1)
                v, i = gal.search(m["q"][:Q], k, idx_offset=off, query_labels=ql[:Q], label_filter=label_filter, exclude=ex[:Q])
                what = f"Q={Q} k={k} {label_filter}"
                _assert_bits(v, wv, what)
                assert (_np(i) == wi).all(), what
    v, i = gal.search(m["q"][:1], 8, query_labels=ql[:1], label_filter="same")
    assert sorted(_np(i)[0, :3].tolist()) == [5, 6, 7] and (_np(i)[0, 3:] == -1).all() and torch.isinf(v[0, 3:]).all()
    with pytest.raises(MI355Error):
        pq.PQGallery(D, DEV, Mq, codebooks=m["cb"]).add(m["x"][:G]).search(m["q"], 3, query_labels=ql, label_filter="same")


# ---- 5. update and training
def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7fffffff), a), np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b).max()


@pytest.mark.parametrize("D,Mq", [(64, 8), (256, 4), (128, 128), (1536, 96), (96, 4)])
def test_update_against_the_float64_mean(D, Mq):
    m = _model(D, Mq)
    n = M.l2_normalize_rows(m["x"])
    codes = torch.from_numpy(m["codes"]).to(DEV)
    want, want_counts = R.update(_np(n), m["codes"], _np(m["cb"]))

    def run():
        g = pq.PQGallery(D, DEV, Mq, codebooks=m["cb"].clone())
        counts = g._update(n, codes)
        return g.codebooks, counts
    cb1, counts = run()
    assert (_np(counts) == want_counts).all() and int(counts.sum()) == GMAX * Mq
    assert _ulps(_np(cb1), want) <= 1
    empty = want_counts == 0
    assert empty.any() and (~empty).any()
    _assert_bits(cb1[torch.from_numpy(empty).to(DEV)], _np(m["cb"])[empty], "an empty cell keeps its centroid")
    M.cosine_topk(m["q"], m["x"], 3)                                 # an unrelated launch in between
    cb2, counts2 = run()
    assert torch.equal(cb1.view(torch.int32), cb2.view(torch.int32)) and torch.equal(counts, counts2)


def test_training_is_deterministic_and_descends():
    n = torch.from_numpy(R.clustered_rows(4096, 64, 40, 0.3, seed=0)).to(DEV)
    a = pq.PQGallery(64, DEV, 8).train(n, iters=5)
    b = pq.PQGallery(64, DEV, 8).train(n, iters=5)
    assert torch.equal(a.codebooks.view(torch.int32), b.codebooks.view(torch.int32)) and torch.equal(a.train_counts, b.train_counts)
    assert int(a.train_counts.sum()) == 4096 * 8
    start = pq.PQGallery(64, DEV, 8).train(n, iters=0)
    assert start.train_counts is None
    pick = M.cluster.seeded_rows(4096, 256, 0)
    nn = _np(M.l2_normalize_rows(n))
    _assert_bits(start.codebooks, nn[pick].reshape(256, 8, 8).transpose(1, 0, 2), "the start is the picked rows' sub-vectors")

    def distortion(g):
        g.add(n)
        d = g.reconstruct().double() - torch.from_numpy(nn).to(DEV).double()
        return float((d * d).sum(dim=1).mean())
    d0, d5 = distortion(start), distortion(a)
    print(f"distortion: {d0:.4f} -> {d5:.4f}")
    assert d5 < d0
    with pytest.raises(MI355Error):
        a.train(n)                                                   # rows are resident now
    g = Gallery(64, DEV).add(n, torch.arange(4096, device=DEV))
    c = pq.PQGallery.from_gallery(g, 8, iters=5)
    assert torch.equal(c.codebooks.view(torch.int32), a.codebooks.view(torch.int32))        # the same rows, the same start
    assert torch.equal(c.codes, a.codes) and torch.equal(c.labels, g.labels) and len(c) == 4096


# ---- 6. the refined search
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D,Mq", [(64, 8), (1536, 96)])
def test_refine_rescoring(D, Mq, dtype):
    m = _model(D, Mq)
    G = 500
    gal = _gallery(m, D, Mq, G)
    exact = Gallery(D, DEV, dtype=dtype).add(m["x"][:G])
    ivf = IVFIndex(exact, M.l2_normalize_rows(m["x"][:1]), torch.zeros(G, dtype=torch.int64, device=DEV))   # one list: every row
    q = m["q"]
    full_v, full_i = ivf.search(q, G, 1)                            # every pair's fp32 dot, in its order
    for k in (3, 150):
        v, i = gal.search(q, k, refine=exact, shortlist=G)
        assert torch.equal(v.view(torch.int32), full_v[:, :k].contiguous().view(torch.int32)) and torch.equal(i, full_i[:, :k])
    dots = np.empty((NQ, G), np.float32)
    np.put_along_axis(dots, _np(full_i), _np(full_v), axis=1)
    for k, short in ((3, 20), (8, 100), (20, 150)):
        _, si = R.topk(m["s"][:, :G], short)                        # the model's shortlist
        mask = np.zeros((NQ, G), bool)
        np.put_along_axis(mask, si, True, axis=1)
        wv, wi = R.topk(dots, k, mask)
        v, i = gal.search(q, k, refine=exact, shortlist=short)
        _assert_bits(v, wv, f"k={k} shortlist={short}")
        assert (_np(i) == wi).all()
    v, i = gal.search(q, 3, refine=exact)                            # the default shortlist: min(max(10 k, 100), 1024, rows)
    v2, i2 = gal.search(q, 3, refine=exact, shortlist=100)
    assert torch.equal(i, i2) and torch.equal(v.view(torch.int32), v2.view(torch.int32))
    v, i = gal.search(q, 3, idx_offset=700, refine=exact, shortlist=100, exclude=i2[:, 0] + 700)
    elig = np.arange(G)[None, :] != _np(i2[:, :1])                  # the best row left out: of the shortlist, then of the result
    _, si = R.topk(m["s"][:, :G], 100, elig)
    mask = np.zeros((NQ, G), bool)
    np.put_along_axis(mask, si, True, axis=1)
    wv, wi = R.topk(dots, 3, mask)
    _assert_bits(v, wv, "exclude with an idx_offset")
    assert (_np(i) == wi + 700).all()
    for kw in ({}, {"refine": exact, "shortlist": 50}):
        mean, per = gal.recall(q, 5, exact, **kw)
        got, want = gal.search(q, 5, **kw)[1], exact.search(q, 5)[1]
        share = np.array([len(set(a) & set(b)) / 5.0 for a, b in zip(_np(got).tolist(), _np(want).tolist())])
        # (the device divides by k as a multiplication with 1 / k: the last bit of 3 / 5 may differ from the host's)
        assert np.abs(_np(per) - share).max() <= 1e-15 and mean == pytest.approx(share.mean(), abs=1e-12)


# ---- 7. side streams
SD, SM = 64, 8


def _stream_gallery():
    cb = _codebooks(SD, SM, 901)
    x = _randn((600, SD), 902)
    return pq.PQGallery(SD, DEV, SM, codebooks=cb).add(x, torch.arange(600, device=DEV) % 7), x


def _pair(shape):
    return {"x": _randn(shape, 903)}, {"x": _randn(shape, 904)}


def _make_train(dev):
    return (lambda i: (lambda g: (g.codebooks, g.train_counts))(pq.PQGallery(SD, dev, SM).train(i["x"], iters=2)),) + _pair((400, SD))


def _make_add(dev):
    cb = _codebooks(SD, SM, 901)

    def op(i):
        g = pq.PQGallery(SD, dev, SM, codebooks=cb, capacity=1).add(i["x"][:100]).add(i["x"][100:])   # grows with rows resident
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


def _make_scores(dev):
    g, _ = _stream_gallery()
    return (lambda i: g.scores(i["x"]),) + _pair((37, SD))


STREAM_CASES = [H.Case("PQGallery.train", ("PQGallery.train",), _make_train, syncs=True),
                H.Case("PQGallery.add", ("PQGallery.add",), _make_add, syncs=True),
                H.Case("PQGallery.search", ("PQGallery.search",), _make_search, syncs=False),
                H.Case("PQGallery.search refined", ("PQGallery.search",), _make_refined, syncs=False),
                H.Case("PQGallery.scores", ("PQGallery.scores",), _make_scores, syncs=False)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
