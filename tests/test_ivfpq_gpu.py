"""IVF-PQ search on the GPU against the NumPy models of the contract BIT FOR BIT: a score is the PQ score (pq_ref.py: table,
scores) of the gallery's own code row, the rows a query sees are those of its probed lists (ivf_ref.py: lists_of, probed_rows,
eligible), and the selection is the library's (gallery_i8_ref.topk with a mask: ties to the lower GALLERY row, pads (-inf, -1)).
Ten hand-made lists whose lengths sit on the edges of the scan's chunk, scattered over the gallery by a seeded permutation, so
that the order of the scan is far from the order of the rows."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import ivf_ref as I
import pq_ref as R
import stream_harness as H
from imageretrievalresearch_amd import Gallery, IVFIndex, MI355Error, ivfpq, pq
from test_ivf_gpu import _planted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = ivfpq.SCAN_CHUNK
LENGTHS = [0, 1, 3, 17, 63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 300]
NLIST, G, NQ = len(LENGTHS), sum(LENGTHS), 200
# (D, M) of tests/test_pq_gpu.py, each another instance: 4-byte code loads with 256 / 256 / 512 threads, 16-byte loads with 512 / 1024
SHAPES = [(4, 4), (64, 8), (176, 44), (192, 48), (1536, 96)]
KS = (1, 3, 8, 9, 150)
E, ONE, THREE, L17, L63, L64, CM1, C, CP1, L300 = range(NLIST)      # the lists by what they hold


def _randn(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_bits(got, want, what=""):
    """float32 arrays equal as int32 bit patterns; a NaN equals any NaN."""
    got, want = np.ascontiguousarray(_np(got), dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.int32)[~gn] == want.view(np.int32)[~wn]).all(), what


def _same(a, b, what=""):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), what


def _assignments():
    """The list of every row: list l has LENGTHS[l] rows, scattered by a seeded permutation."""
    a = np.empty(G, np.int64)
    a[np.random.RandomState(5).permutation(G)] = np.repeat(np.arange(NLIST), LENGTHS)
    return a


_models = {}


def _model(D, Mq):
    """Seeded rows, queries, codebooks and centroids of one shape; the rows encoded on the GPU (the encoder is tested elsewhere),
    the model's scores of every (query, row) pair from the codes read back, and the index over the hand-made lists."""
    key = (D, Mq)
    if key not in _models:
        x, q = _randn((G, D), 100 + D + Mq), _randn((NQ, D), 200 + D + Mq)
        cb = (_randn((Mq, 256, D // Mq), 300 + D + Mq) / float(np.sqrt(D))).contiguous()
        lab = torch.randint(0, 4, (G,), generator=torch.Generator().manual_seed(D)).to(DEV)
        gal = pq.PQGallery(D, DEV, Mq, codebooks=cb).add(x, lab)
        assign = _assignments()
        ix = ivfpq.IVFPQIndex(gal, _randn((NLIST, D), 400 + D + Mq), _dev(assign))
        offsets, order = I.lists_of(assign, NLIST)
        assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
        assert (np.abs(order - np.arange(G)) > G // 8).mean() > 0.5              # far from the identity
        s = R.scores(R.table(_np(M.l2_normalize_rows(q)), _np(cb)), _np(gal.codes))
        _models[key] = dict(x=x, q=q, gal=gal, ix=ix, s=s, offsets=offsets, order=order, lab=_np(lab), top={})
    return _models[key]


def _probed_mask(m, probes):
    mask = np.zeros((probes.shape[0], G), bool)
    for qi, p in enumerate(probes):
        mask[qi, I.probed_rows(m["offsets"], m["order"], p)] = True
    return mask


def _rot(lists, n=NQ):
    """(n, len(lists)): query q probes ``lists`` rotated by q: the same rows, another scan order."""
    lists = np.asarray(lists, np.int64)
    return np.stack([np.roll(lists, -qi) for qi in range(n)])


# Probe sets (NQ, nprobe); a test takes the first Q rows
PROBES = {
    "only the empty list": np.full((NQ, 1), E, np.int64),
    "fewer rows than k": _rot([E, ONE, THREE]),
    "a list boundary at a chunk edge": np.tile(np.array([CM1, ONE, L300, L17], np.int64), (NQ, 1)),
    "a list of exactly one chunk": np.tile(np.array([C, THREE, L63], np.int64), (NQ, 1)),
    "a list straddling two chunks": np.tile(np.array([CP1, L64, L17], np.int64), (NQ, 1)),
    "nprobe = 1": (np.arange(NQ, dtype=np.int64) % NLIST)[:, None],
    "nprobe = nlist": _rot(np.random.RandomState(6).permutation(NLIST)),
    # short queries (their workgroups leave early) beside queries that fill three chunks
    "queries of different lengths": np.array([[[E, ONE, THREE], [CM1, C, CP1], [L17, E, L63], [CP1, L300, CM1], [THREE, L64, ONE]][qi % 5]
                                              for qi in range(NQ)], np.int64),
}


def _want(m, name):
    """The model's top-150 of every query over its probed rows, once per probe set: a smaller k and a smaller Q are prefixes."""
    if name not in m["top"]:
        m["top"][name] = R.topk(m["s"], max(KS), _probed_mask(m, PROBES[name]))
    return m["top"][name]


# ---- 1. model equality
@pytest.mark.parametrize("D,Mq", SHAPES)
def test_search_equals_the_model(D, Mq):
    m = _model(D, Mq)
    ix = m["ix"]
    for name, probes in PROBES.items():
        wv, wi = _want(m, name)
        if name == "fewer rows than k":
            assert (wi[:, :4] >= 0).all() and (wi[:, 4:] == -1).all()
        if name == "only the empty list":
            assert (wi == -1).all() and np.isinf(wv).all()
        for Q in (1, 3, NQ):
            p = _dev(probes[:Q])
            for k in KS:
                v, i = ix.search(m["q"][:Q], k, probes=p)
                what = f"D={D} M={Mq} {name} Q={Q} k={k}"
                _assert_bits(v, wv[:Q, :k], what)
                assert (_np(i) == wi[:Q, :k]).all(), what
    one, many = ix.search(m["q"][:1], 8, probes=_dev(PROBES["nprobe = nlist"][:1])), ix.search(m["q"], 8, probes=_dev(PROBES["nprobe = nlist"]))
    _same(one, (many[0][:1].contiguous(), many[1][:1].contiguous()), "not on Q")


@pytest.mark.parametrize("D,Mq", [(64, 8), (192, 48)])
def test_more_queries_than_one_block(D, Mq):
    """300 queries are two launches of the scan (256 + 44): the second block's probes, filter and output rows begin at its first
    query.  A row's result does not depend on the batch it came in, so the model is the 200 queries' own."""
    m = _model(D, Mq)
    ix, off = m["ix"], 300
    pick = np.concatenate([np.arange(NQ), np.arange(100)[::-1]])                     # 300 queries: rows 256.. are 43, 42, ...
    probes = PROBES["queries of different lengths"][(pick * 7) % NQ]                 # every query with another query's probes
    probed = _probed_mask(m, probes)
    q = m["q"][_dev(pick)]
    ql = pick % 4
    ex = np.where(pick % 3 == 1, -1, R.topk(m["s"][pick], 1, probed)[1][:, 0] + off)
    ok = I.eligible(G, 300, ql, m["lab"], "different", ex, off)
    for k in (8, 150):
        wv, wi = R.topk(m["s"][pick], k, probed)
        v, i = ix.search(q, k, probes=_dev(probes))
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all(), f"k={k}"
        wv, wi = R.topk(m["s"][pick], k, probed & ok)
        v, i = ix.search(q, k, probes=_dev(probes), idx_offset=off, query_labels=_dev(ql), label_filter="different", exclude=_dev(ex))
        _assert_bits(v, wv, f"k={k} filtered")
        assert (_np(i) == np.where(wi >= 0, wi + off, -1)).all(), f"k={k} filtered"


# ---- 2. every list probed = the exhaustive search
@pytest.mark.parametrize("D,Mq", SHAPES)
def test_every_list_probed_equals_the_exhaustive_search(D, Mq):
    m = _model(D, Mq)
    ix, gal, q = m["ix"], m["gal"], m["q"]
    ql = torch.randint(0, 4, (NQ,), generator=torch.Generator().manual_seed(D + 1)).to(DEV)
    ex = (torch.arange(NQ, device=DEV) * 31 % G) + 7000
    ex[1] = -1
    for k in (3, 8, 150):
        _same(ix.search(q, k, nprobe=NLIST), gal.search(q, k), f"k={k}")
        _same(ix.search(q, k, nprobe=NLIST, idx_offset=7000), gal.search(q, k, idx_offset=7000), f"k={k} idx_offset")
        for label_filter in ("same", "different", None):
            kw = dict(query_labels=ql, label_filter=label_filter, exclude=ex, idx_offset=7000)
            _same(ix.search(q, k, nprobe=NLIST, **kw), gal.search(q, k, **kw), f"k={k} {label_filter}")
    _same(ix.search(q[:1], 8, nprobe=NLIST), gal.search(q[:1], 8), "Q=1")


# ---- 3. ties across lists
def test_ties_go_to_the_lower_gallery_row_whatever_the_scan_order():
    D, Mq = 64, 8
    m = _model(D, Mq)
    x = m["x"][:500]
    gal = pq.PQGallery(D, DEV, Mq, codebooks=m["gal"].codebooks).add(x).add(x)       # rows r and r + 500 are twins
    s = R.scores(R.table(_np(M.l2_normalize_rows(m["q"])), _np(gal.codebooks)), _np(gal.codes))
    assign = np.concatenate([np.ones(500, np.int64), np.zeros(500, np.int64)])       # list 0 holds the HIGHER rows
    ix = ivfpq.IVFPQIndex(gal, _randn((2, D), 1), _dev(assign))
    probes = _dev(np.tile(np.array([0, 1], np.int64), (NQ, 1)))                     # ... and is scanned first
    for k in (8, 150):
        v, i = ix.search(m["q"], k, probes=probes)
        wv, wi = R.topk(s, k)
        _assert_bits(v, wv, f"k={k}")
        assert (_np(i) == wi).all()
        assert torch.equal(v[:, 0::2].view(torch.int32), v[:, 1::2].view(torch.int32))      # the two copies score the same bits
        first, second = _np(i[:, 0::2]), _np(i[:, 1::2])
        assert (first < second).all() and (first + 500 == second).sum() > 0.9 * first.size
        v2, i2 = ix.search(m["q"], k, probes=probes, idx_offset=10 ** 6)
        assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(i2, i + 10 ** 6)


# ---- 4. filters
@pytest.mark.parametrize("D,Mq", [(64, 8), (1536, 96)])
def test_filters_go_by_gallery_row(D, Mq):
    m = _model(D, Mq)
    ix, off = m["ix"], 5000
    probes = PROBES["queries of different lengths"]
    probed = _probed_mask(m, probes)
    ql = np.arange(NQ) % 4
    unfiltered = R.topk(m["s"], 1, probed)[1][:, 0]
    ex = np.where(np.arange(NQ) % 3 == 1, -1, unfiltered + off)                      # two thirds leave their best probed row out
    for label_filter in ("same", "different", None):
        ok = I.eligible(G, NQ, ql, m["lab"], label_filter, ex, off)
        for k in (3, 8, 150):
            wv, wi = R.topk(m["s"], k, probed & ok)
            wi = np.where(wi >= 0, wi + off, -1)
            for Q in (1, NQ):
                v, i = ix.search(m["q"][:Q], k, probes=_dev(probes[:Q]), idx_offset=off, query_labels=_dev(ql[:Q]),
                                 label_filter=label_filter, exclude=_dev(ex[:Q]))
                what = f"Q={Q} k={k} {label_filter}"
                _assert_bits(v, wv[:Q], what)
                assert (_np(i) == wi[:Q]).all(), what
    with pytest.raises(MI355Error):
        ivfpq.IVFPQIndex(pq.PQGallery(D, DEV, Mq, codebooks=m["gal"].codebooks).add(m["x"]), ix.centroids, ix.assignments) \
            .search(m["q"], 3, 2, query_labels=_dev(ql), label_filter="same")             # no gallery labels


# ---- 5. refine
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D,Mq", [(64, 8), (1536, 96)])
def test_refine_rescoring(D, Mq, dtype):
    m = _model(D, Mq)
    ix, q = m["ix"], m["q"]
    exact = Gallery(D, DEV, dtype=dtype).add(m["x"])
    # every pair's fp32 dot from the routine the refinement shares (one IVF list that holds every row; its slab is in row order)
    one = IVFIndex(exact, M.l2_normalize_rows(m["x"][:1]), torch.zeros(G, dtype=torch.int64, device=DEV))
    cv, ci = one._scan(q, torch.zeros((NQ, 1), dtype=torch.int64, device=DEV), G, 0, None)
    assert (_np(ci) == np.arange(G)[None, :]).all()
    dots32 = _np(cv)
    dots64 = _np(M.l2_normalize_rows(q)).astype(np.float64) @ _np(exact.data.float()).astype(np.float64).T
    for name, k, short in (("queries of different lengths", 3, 20), ("a list straddling two chunks", 8, 100),
                           ("nprobe = nlist", 20, 150), ("fewer rows than k", 3, 50)):
        p = _dev(PROBES[name])
        si = _np(ix.search(q, short, probes=p)[1])                   # the unrefined shortlist
        v, i = ix.search(q, k, probes=p, refine=exact, shortlist=short)
        wi = np.full((NQ, k), -1, np.int64)
        wv = np.full((NQ, k), -np.inf, np.float32)
        for qi in range(NQ):
            c = si[qi][si[qi] >= 0]
            c = c[np.lexsort((c, -dots64[qi, c]))][:k]               # by the float64 dot, then the lower row
            wi[qi, :c.size], wv[qi, :c.size] = c, dots32[qi, c]
        what = f"{name} k={k} shortlist={short}"
        assert (_np(i) == wi).all(), what
        _assert_bits(v, wv, what)                                    # as tests/test_pq_gpu.py::test_refine_rescoring: the routine's bits
    p = _dev(PROBES["nprobe = nlist"])
    for k in (3, 150):                                               # every list, the longest shortlist: the routine's own order
        v, i = ix.search(q, k, probes=p, refine=exact, shortlist=1024)
        pv, pi = m["gal"].search(q, k, refine=exact, shortlist=1024)
        assert torch.equal(v.view(torch.int32), pv.view(torch.int32)) and torch.equal(i, pi)
    v, i = ix.search(q, 3, probes=p, refine=exact)                   # the default shortlist: min(max(10 k, 100), 1024, rows)
    v2, i2 = ix.search(q, 3, probes=p, refine=exact, shortlist=100)
    assert torch.equal(i, i2) and torch.equal(v.view(torch.int32), v2.view(torch.int32))


# ---- 6. planted clusters need one probe
@pytest.mark.parametrize("Mq", [8, 16])
def test_planted_clusters_need_one_probe(Mq):
    centres, lab, x, qlab, qs = _planted()
    xt, q = _dev(x), _dev(qs)
    # the model first: the planted structure survives the codes, certified before the GPU result is looked at
    nn = _np(M.l2_normalize_rows(xt))
    cb, _ = R.lloyd(nn, Mq, 3, M.cluster.seeded_rows(320, 256, 0))
    s = R.scores(R.table(_np(M.l2_normalize_rows(q)), cb), R.encode(nn, cb))
    own_worst = np.array([s[qi, lab == qlab[qi]].min() for qi in range(24)])
    other_best = np.array([s[qi, lab != qlab[qi]].max() for qi in range(24)])
    print(f"M={Mq}: margin {float((own_worst - other_best).min()):.3f}")
    assert (own_worst - other_best).min() > 0.5
    assert (lab[R.topk(s, 5)[1]] == qlab[:, None]).all()
    gal = pq.PQGallery(64, DEV, Mq).train(xt, iters=3).add(xt)
    ix = ivfpq.IVFPQIndex.build(gal, xt, 8, init=_dev(centres))
    assert (_np(ix.assignments) == lab).all()                        # the lists are the planted clusters
    offsets, order = I.lists_of(lab, 8)
    assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
    assert (_np(ix.list_codes) == _np(gal.codes)[order]).all()
    _same(ix.search(q, 5, nprobe=1), gal.search(q, 5), "one probe")
    mean, per = ix.recall(q, 5, 1)
    assert mean == 1.0 and per.shape == (24,) and bool((per == 1.0).all())
    g = Gallery(64, DEV).add(xt)
    same = gal.ivf(g, 8, init=_dev(centres))                         # the convenience, over the Gallery of the same rows
    assert torch.equal(same.assignments, ix.assignments) and torch.equal(same.list_codes, ix.list_codes)
    mean, per = ix.recall(q, 5, 1, exact=g)                          # lists and codes together: what the codes lose alone
    want = gal.recall(q, 5, g)
    assert mean == want[0] and torch.equal(per, want[1])
    both = ivfpq.IVFPQIndex.from_gallery(g, Mq, 8, pq_iters=3, iters=2)
    assert torch.equal(both.pq.codes, gal.codes) and both.nlist == 8 and len(both.pq) == 320


# ---- 7. add and staleness
def test_add_and_staleness():
    D, Mq = 64, 8
    m = _model(D, Mq)
    x, q = m["x"], m["q"]
    gal = pq.PQGallery(D, DEV, Mq, codebooks=m["gal"].codebooks).add(x[:4000], torch.arange(4000, device=DEV) % 4)
    ix = ivfpq.IVFPQIndex.build(gal, x[:4000], 12, iters=2)
    old = ix.assignments.clone()
    new = x[4000:6000]
    assert ix.add(new, torch.arange(2000, device=DEV) % 4) is ix and not ix.stale and len(gal) == 6000 == ix.rows
    assert torch.equal(ix.assignments[:4000], old)
    assert torch.equal(ix.assignments[4000:], M.assign_clusters(new, ix.centroids)[0])
    offsets, order = I.lists_of(_np(ix.assignments), 12)
    assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
    assert (_np(ix.list_codes) == _np(gal.codes)[order]).all() and (_np(ix.counts) == np.diff(offsets)).all()
    for k in (3, 150):
        _same(ix.search(q, k, nprobe=12), gal.search(q, k), f"k={k}")
    ql = torch.arange(NQ, device=DEV) % 4
    _same(ix.search(q, 8, nprobe=12, query_labels=ql, label_filter="same"), gal.search(q, 8, query_labels=ql, label_filter="same"))
    assert ix.nbytes == 12 * D * 4 + 8 * (6000 + 13 + 6000 + 12) + 6000 * Mq
    assert ix.add(x[:0]) is ix and ix.rows == 6000                   # nothing to add
    gal.add(x[6000:6001])                                            # behind the index's back
    assert ix.stale
    with pytest.raises(MI355Error, match="stale"):
        ix.search(q, 3, nprobe=2)
    with pytest.raises(MI355Error, match="stale"):
        ix.add(x[:1])


# ---- 8. side streams
SD, SM = 64, 8


def _stream_index():
    cb = (_randn((SM, 256, SD // SM), 901) / 8.0).contiguous()
    x = _randn((3000, SD), 902)
    gal = pq.PQGallery(SD, DEV, SM, codebooks=cb).add(x, torch.arange(3000, device=DEV) % 7)
    return ivfpq.IVFPQIndex.build(gal, x, 6, iters=2), x


def _pair(shape):
    return {"x": _randn(shape, 903)}, {"x": _randn(shape, 904)}


def _make_build(dev):
    cb = (_randn((SM, 256, SD // SM), 901) / 8.0).contiguous()

    def op(i):
        ix = pq.PQGallery(SD, dev, SM, codebooks=cb).add(i["x"]).ivf(i["x"], 6, iters=2)
        return ix.centroids, ix.assignments, ix.offsets, ix.order, ix.list_codes
    return (op,) + _pair((1500, SD))


def _make_search(dev):
    ix, _ = _stream_index()
    return (lambda i: (ix.search(i["x"], 3, 2), ix.search(i["x"], 150, 3), ix.search(i["x"], 8, nprobe=6)),) + _pair((37, SD))


def _make_filtered(dev):
    ix, _ = _stream_index()
    ql, ex = torch.arange(37, device=dev) % 7, torch.arange(37, device=dev) * 5
    return (lambda i: (ix.search(i["x"], 8, 3, query_labels=ql, label_filter="different", exclude=ex),
                       ix.search(i["x"], 20, 3, query_labels=ql, label_filter="same")),) + _pair((37, SD))


def _make_refined(dev):
    ix, x = _stream_index()
    f32, f16 = Gallery(SD, dev).add(x), Gallery(SD, dev, dtype=torch.float16).add(x)
    return (lambda i: (ix.search(i["x"], 5, 3, refine=f32), ix.search(i["x"], 5, 3, refine=f16, shortlist=64)),) + _pair((37, SD))


def _make_add(dev):
    cb = (_randn((SM, 256, SD // SM), 901) / 8.0).contiguous()
    x = _randn((1000, SD), 902)
    cen = _randn((6, SD), 905)
    a = torch.arange(1000, device=dev) % 6

    def op(i):
        ix = ivfpq.IVFPQIndex(pq.PQGallery(SD, dev, SM, codebooks=cb).add(x), cen, a).add(i["x"])
        return ix.assignments, ix.offsets, ix.order, ix.list_codes
    return (op,) + _pair((700, SD))


def _make_probe(dev):
    ix, _ = _stream_index()
    return (lambda i: ix.probe(i["x"], 3),) + _pair((37, SD))


STREAM_CASES = [H.Case("IVFPQIndex.build", ("IVFPQIndex.build", "PQGallery.ivf"), _make_build, syncs=True),
                H.Case("IVFPQIndex.search", ("IVFPQIndex.search",), _make_search, syncs=True),
                H.Case("IVFPQIndex.search filtered", ("IVFPQIndex.search",), _make_filtered, syncs=True),
                H.Case("IVFPQIndex.search refined", ("IVFPQIndex.search",), _make_refined, syncs=True),
                H.Case("IVFPQIndex.add", ("IVFPQIndex.add",), _make_add, syncs=True),
                H.Case("IVFPQIndex.probe", ("IVFPQIndex.probe",), _make_probe, syncs=False)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
