"""Residual IVF-PQ on the GPU against the NumPy model of the contract (ivfrpq_ref.py on pq_ref.py) BIT FOR BIT: the residual
rows, the codes, the trained codebooks, and the score ``float32(coarse + PQ score)`` of every (query, row) pair with the top-k
over the probed lists (ties to the lower GALLERY row, pads (-inf, -1)).  The coarse terms the model adds are read from
``index.coarse`` (the rescoring routine over the centroids, itself checked against float64 and against the C entry), so a search
that matches the model has added exactly that term, of the row's own list, inside the scan.
Six hand-made lists of lengths [0, 2048, 1, 0, 700, 251] over 3000 rows scattered by a seeded permutation: one list ends on the
scan's 2048-position chunk edge, empty lists come first and in between, one list holds one row."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import ivf_ref as I
import ivfrpq_ref as V
import pq_ref as R
import stream_harness as H
from helpers import SCORE_TOL
from imageretrievalresearch_amd import Gallery, MI355Error, _lib, cluster, ivfrpq, pq, rank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [0, 2048, 1, 0, 700, 251]
NLIST, G = len(LENGTHS), sum(LENGTHS)
# (D, M): 256 threads with 4-byte code loads, 256 / 512 / 1024 threads with 16-byte loads
SHAPES = [(32, 8), (64, 16), (192, 48), (384, 96)]
KS = (1, 3, 8, 9, 150)
NQ = {(32, 8): 257}                                     # the query-block edge is tested at (32, 8); 40 queries elsewhere
Index = ivfrpq.ResidualIVFPQIndex


def _randn(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_bits(got, want, what=""):
    """float32 arrays equal as int32 bit patterns; a NaN equals any NaN."""
    got = np.ascontiguousarray(_np(got) if torch.is_tensor(got) else got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.int32)[~gn] == want.view(np.int32)[~wn]).all(), what


def _same(a, b, what=""):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), what


def _assignments():
    a = np.empty(G, np.int64)
    a[np.random.RandomState(5).permutation(G)] = np.repeat(np.arange(NLIST), LENGTHS)
    return a


def _all_lists(Q):
    return np.tile(np.arange(NLIST, dtype=np.int64), (Q, 1))


_models = {}


def _model(D, Mq):
    """Seeded rows, queries, unit centroids, random codebooks and labels of one shape; the index over the hand-made lists; the
    model's residuals and codes (checked against the index's, bit for bit) and its score of every (query, row) pair."""
    key = (D, Mq)
    if key not in _models:
        nq = NQ.get(key, 40)
        x, q = _randn((G, D), 100 + D + Mq), _randn((nq, D), 200 + D + Mq)
        cen = M.l2_normalize_rows(_randn((NLIST, D), 400 + D + Mq))
        cb = (_randn((Mq, 256, D // Mq), 300 + D + Mq) / float(np.sqrt(D))).contiguous()
        lab = torch.randint(0, 4, (G,), generator=torch.Generator().manual_seed(D)).to(DEV)
        assign = _assignments()
        ix = Index(cen, cb).add(x, lab, assignments=_dev(assign))
        offsets, order = I.lists_of(assign, NLIST)
        assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all() and (_np(ix.counts) == LENGTHS).all()
        nn, qn = _np(M.l2_normalize_rows(x)), _np(M.l2_normalize_rows(q))
        codes = V.encode(nn, assign, _np(cen), _np(cb))
        assert (_np(ix.codes) == codes).all() and (_np(ix.list_codes) == codes[order]).all()
        coarse = _np(ix.coarse(q, _dev(_all_lists(nq))))
        s = V.scores(coarse, qn, _np(cb), codes, assign)
        _models[key] = dict(x=x, q=q, nq=nq, ix=ix, s=s, assign=assign, cen=cen, cb=cb, qn=qn, nn=nn, codes=codes, coarse=coarse,
                            lab=_np(lab))
    return _models[key]


def _want(m, k, probes, **filt):
    return V.search(m["s"][: len(probes)], k, m["assign"], NLIST, probes, **filt)


PROBES = {
    "a chunk edge on a list edge, then an empty list": [1, 2, 3, 4],
    "a list straddles the chunk edge, not nearest first": [4, 1, 5],
    "only empty lists": [0, 3],
    "every list": [5, 4, 3, 2, 1, 0],
}


# ---- 1. model equality
@pytest.mark.parametrize("D,Mq", SHAPES)
def test_search_equals_the_model(D, Mq):
    m = _model(D, Mq)
    ix, nq = m["ix"], m["nq"]
    for name, lists in PROBES.items():
        probes = np.tile(np.array(lists, np.int64), (nq, 1))
        wv, wi = _want(m, max(KS), probes)
        if name == "only empty lists":
            assert (wi == -1).all() and np.isneginf(wv).all()
        if name == "every list":
            ev, ei = R.topk(m["s"], max(KS))
            assert (ei == wi).all() and (ev.view(np.int32) == wv.view(np.int32)).all()      # the model's exhaustive top-k
        for Q in (1, nq):
            for k in KS:
                v, i = ix.search(m["q"][:Q], k, probes=_dev(probes[:Q]))
                what = f"D={D} M={Mq} {name} Q={Q} k={k}"
                assert (_np(i) == wi[:Q, :k]).all(), what
                _assert_bits(v, wv[:Q, :k], what)
    picked = _np(ix.probe(m["q"], 2))                                  # nprobe=: the lists of probe()
    for k in (3, 150):
        wv, wi = _want(m, k, picked)
        v, i = ix.search(m["q"], k, nprobe=2)
        assert (_np(i) == wi).all(), f"nprobe=2 k={k}"
        _assert_bits(v, wv, f"nprobe=2 k={k}")


# ---- 2. the second query block
def _rotating_probes(nq):
    """Query q probes three of the lists [1, 4, 5, 2], rotated by q: every query its own order and its own coarse terms."""
    return np.stack([np.roll(np.array([1, 4, 5, 2], np.int64), -qi)[:3] for qi in range(nq)])


def test_query_block_edge():
    """257 queries are two launches (256 + 1): query 256 begins the second block, whose coarse terms, bases, probes and filter
    must be its own."""
    m = _model(32, 8)
    ix, nq, off = m["ix"], m["nq"], 900
    assert nq == 257
    probes = _rotating_probes(nq)
    ql = np.arange(nq) % 4
    # two thirds leave their best row out, query 256 among them
    ex = np.where(np.arange(nq) % 3 == 2, -1, _want(m, 1, probes)[1][:, 0] + off)
    filt = dict(query_labels=ql, gallery_labels=m["lab"], label_filter="different", exclude=ex, idx_offset=off)
    for k in (3, 9):
        wv, wi = _want(m, k, probes)
        fv, fi = _want(m, k, probes, **filt)
        assert (fi[256] != wi[256] + off).any()                        # the filter changes the last query's answer
        for Q in (1, 5, 257):
            v, i = ix.search(m["q"][:Q], k, probes=_dev(probes[:Q]))
            assert (_np(i) == wi[:Q]).all(), f"k={k} Q={Q}"
            _assert_bits(v, wv[:Q], f"k={k} Q={Q}")
            v, i = ix.search(m["q"][:Q], k, probes=_dev(probes[:Q]), idx_offset=off, query_labels=_dev(ql[:Q]),
                             label_filter="different", exclude=_dev(ex[:Q]))
            assert (_np(i) == fi[:Q]).all(), f"k={k} Q={Q} filtered"
            _assert_bits(v, fv[:Q], f"k={k} Q={Q} filtered")


# ---- 3. one score per pair
def test_coarse_is_the_rescoring_routine_over_the_centroids():
    m = _model(192, 48)
    ix, q, nq = m["ix"], m["q"], m["nq"]
    probes = _dev(_rotating_probes(nq))
    got = ix.coarse(q, probes)
    L = _lib.lib()
    direct = torch.empty((nq, 3), dtype=torch.float32, device=DEV)
    ws = torch.empty(L.mi355_rescore_candidates_workspace_bytes(nq, 192), dtype=torch.uint8, device=DEV)
    _lib.check(L.mi355_rescore_candidates(q.data_ptr(), nq, 192, ix.pq.eps, m["cen"].data_ptr(), _lib.DTYPE_F32, 192, NLIST,
                                          probes.data_ptr(), 3, 0, direct.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(torch.device(DEV))))
    assert torch.equal(got.view(torch.int32), direct.view(torch.int32))
    want = np.take_along_axis(m["qn"].astype(np.float64) @ _np(m["cen"]).astype(np.float64).T, _np(probes), axis=1)
    assert np.abs(_np(got) - want).max() < SCORE_TOL
    _assert_bits(got, np.take_along_axis(m["coarse"], _np(probes), axis=1))           # a term does not depend on the probe set


@pytest.mark.parametrize("D,Mq", [(32, 8), (384, 96)])
def test_one_score_per_pair(D, Mq):
    """The value of a (query, row) pair is float32(coarse[q][list of the row] + the model's PQ sum) whatever the search: nprobe = 1,
    3 or every list, k = 3 or 150, Q = 1 or all queries, with and without a filter."""
    m = _model(D, Mq)
    ix, q, nq, s = m["ix"], m["q"], m["nq"], m["s"]
    bits, seen = s.view(np.int32), set()

    def record(v, i, rows, off=0):
        """Every returned (query, row) pair carries the model's bits for that pair."""
        v, i = _np(v).view(np.int32), _np(i)
        qi = np.broadcast_to(np.asarray(rows)[:, None], i.shape)
        real = i >= 0
        assert (v[real] == bits[qi[real], i[real] - off]).all()
        seen.update((qi[real] * G + i[real] - off).tolist())

    every = np.arange(nq)
    for lists in ([4], [4, 1, 5], [5, 4, 3, 2, 1, 0]):
        p = np.tile(np.array(lists, np.int64), (nq, 1))
        for k in (3, 150):
            record(*ix.search(q, k, probes=_dev(p)), every)
            for qi in (0, nq - 1):
                record(*ix.search(q[qi: qi + 1], k, probes=_dev(p[:1])), [qi])
        best = _np(ix.search(q, 1, probes=_dev(p))[1])[:, 0]
        record(*ix.search(q, 150, probes=_dev(p), exclude=_dev(best + 7), idx_offset=7), every, 7)
        record(*ix.search(q, 3, probes=_dev(p), query_labels=_dev(np.arange(nq) % 4), label_filter="same"), every)
    assert len(seen) > 150 * nq                                        # (the three probe sets share list 4's rows)


# ---- 4. ties
def test_ties_go_to_the_lower_gallery_row():
    D, Mq = 64, 16
    m = _model(D, Mq)
    x, q, nq = m["x"][:500], m["q"], m["nq"]
    cen = m["cen"][:2].contiguous()
    a = np.arange(500) % 2
    a2 = np.concatenate([a, a])                                        # rows r and r + 500 are twins in one list
    ix = Index(cen, m["cb"]).add(torch.cat([x, x]), assignments=_dev(a2))
    codes = _np(ix.codes)
    assert (codes[:500] == codes[500:]).all()
    s = V.scores(_np(ix.coarse(q, _dev(np.tile(np.arange(2), (nq, 1))))), m["qn"], _np(m["cb"]), codes, a2)
    probes = _dev(np.tile(np.array([1, 0], np.int64), (nq, 1)))
    for k in (8, 150):
        v, i = ix.search(q, k, probes=probes)
        wv, wi = R.topk(s, k)
        assert (_np(i) == wi).all()
        _assert_bits(v, wv, f"k={k}")
        assert torch.equal(v[:, 0::2].view(torch.int32), v[:, 1::2].view(torch.int32))
        first, second = _np(i[:, 0::2]), _np(i[:, 1::2])
        assert (first < second).all() and (first + 500 == second).sum() > 0.9 * first.size


# ---- 5. filters
@pytest.mark.parametrize("D,Mq", [(64, 16), (384, 96)])
def test_filters_go_by_gallery_row(D, Mq):
    m = _model(D, Mq)
    ix, nq, off = m["ix"], m["nq"], 5000
    probes = _rotating_probes(nq)
    ql = np.arange(nq) % 4
    ex = np.where(np.arange(nq) % 3 == 1, -1, _want(m, 1, probes)[1][:, 0] + off)
    for label_filter in ("same", "different", None):
        filt = dict(query_labels=ql, gallery_labels=m["lab"], label_filter=label_filter, exclude=ex, idx_offset=off)
        for k in (3, 8, 150):
            wv, wi = _want(m, k, probes, **filt)
            for Q in (1, nq):
                v, i = ix.search(m["q"][:Q], k, probes=_dev(probes[:Q]), idx_offset=off, query_labels=_dev(ql[:Q]),
                                 label_filter=label_filter, exclude=_dev(ex[:Q]))
                what = f"Q={Q} k={k} {label_filter}"
                assert (_np(i) == wi[:Q]).all(), what
                _assert_bits(v, wv[:Q], what)
    one = np.tile(np.array([2, 0], np.int64), (nq, 1))                 # the one-row list: fewer eligible rows than k
    the_row = int(np.nonzero(m["assign"] == 2)[0][0])
    for k in (3, 9):
        v, i = ix.search(m["q"], k, probes=_dev(one), query_labels=_dev(ql), label_filter="same")
        wv, wi = _want(m, k, one, query_labels=ql, gallery_labels=m["lab"], label_filter="same")
        assert (_np(i) == wi).all() and (wi[:, 1:] == -1).all() and set(wi[:, 0]) == {-1, the_row}
        _assert_bits(v, wv)
    with pytest.raises(MI355Error):
        Index(m["cen"], m["cb"]).add(m["x"][:300]).search(m["q"], 3, 2, query_labels=_dev(ql), label_filter="same")   # no gallery labels


def test_a_list_id_outside_the_lists_is_refused_after_the_call():
    """Such a list counts as empty: no centroid is read for it (its coarse term is -inf and never used) and the flag is raised."""
    m = _model(32, 8)
    ix, q = m["ix"], m["q"][:5]
    for bad in (NLIST, -1):
        probes = _dev(np.tile(np.array([4, bad, 1], np.int64), (5, 1)))
        assert bool(torch.isneginf(ix.coarse(q, probes)[:, 1]).all())
        for k in (3, 9):
            with pytest.raises(MI355Error, match=r"a list id outside \[0, nlist=6\)"):
                ix.search(q, k, probes=probes)
    good = _dev(np.tile(np.array([4, 1], np.int64), (5, 1)))
    wv, wi = _want(m, 3, _np(good))
    v, i = ix.search(q, 3, probes=good)                                # the index is as usable as before
    assert (_np(i) == wi).all()
    _assert_bits(v, wv)


# ---- 6. refine
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_refine_rescoring(dtype):
    D, Mq = 64, 16
    m = _model(D, Mq)
    ix, q, nq = m["ix"], m["q"], m["nq"]
    exact = Gallery(D, DEV, dtype=dtype).add(m["x"])
    qc = q.contiguous()
    for lists, k, short in (([4, 1, 5], 3, 20), ([1, 2, 3, 4], 8, 100), ([5, 4, 3, 2, 1, 0], 20, 150), ([2, 0], 3, 50)):
        probes = np.tile(np.array(lists, np.int64), (nq, 1))
        cand = _dev(_want(m, short, probes)[1])                       # the model's shortlist, through the existing entry
        wv, wi = pq._refined_topk(ix.pq, qc, torch.empty((nq, short), dtype=torch.float32, device=DEV), cand, k, exact, 0)
        v, i = ix.search(q, k, probes=_dev(probes), refine=exact, shortlist=short)
        assert torch.equal(i, wi) and torch.equal(v.view(torch.int32), wv.view(torch.int32)), (lists, k, short)
    p = _dev(np.tile(np.array([4, 1], np.int64), (nq, 1)))
    _same(ix.search(q, 3, probes=p, refine=exact), ix.search(q, 3, probes=p, refine=exact, shortlist=100), "the default shortlist")


# ---- 7. the residual kernel
@pytest.mark.parametrize("D", [32, 30, 1536])                         # 16-byte lanes; scalar lanes; more than one load per lane
def test_residual_rows(D):
    n, nlist = 1027, 5                                                # not a multiple of the 4 rows of a workgroup
    x, cen = _randn((n, D), 11 + D), M.l2_normalize_rows(_randn((nlist, D), 12 + D))
    a = torch.randint(0, nlist, (n,), generator=torch.Generator().manual_seed(D)).to(DEV)
    nn = M.l2_normalize_rows(x)
    want = V.residuals(_np(nn), _np(a), _np(cen))
    out = torch.full((n + 1, D), 7.0, device=DEV)
    _assert_bits(ivfrpq._residuals(x, False, a, cen, rank._EPS, out[:n]), want, "raw rows")
    assert bool((out[n] == 7.0).all())                                 # nothing past the last row
    _assert_bits(ivfrpq._residuals(nn, True, a, cen, rank._EPS, torch.empty_like(x)), want, "normalised rows")
    _assert_bits(ivfrpq._residuals(nn.clone(), True, a, cen, rank._EPS, out[:n]), want)
    inplace = nn.clone()
    _assert_bits(ivfrpq._residuals(inplace, True, a, cen, rank._EPS, inplace), want, "in place")
    for bad in (nlist, -1):
        b = a.clone()
        b[1000] = bad
        with pytest.raises(MI355Error, match=r"an assignment outside \[0, nlist=5\)"):
            ivfrpq._residuals(nn, True, b, cen, rank._EPS, torch.empty_like(x))


# ---- 8. build
def test_build_equals_kmeans_then_the_models_lloyd():
    N, D, Mq, nlist = 1024, 32, 8, 8
    x = _dev(R.clustered_rows(N, D, 8, 0.4, 3)) * 2.5                  # raw rows: not unit length
    lab = torch.arange(N, device=DEV) % 5
    ix = Index.build(x, Mq, nlist, labels=lab, iters=4, pq_iters=3, seed=1)
    km = cluster.spherical_kmeans(x, nlist, iters=4, seed=1)
    assert torch.equal(ix.centroids.view(torch.int32), km.centroids.view(torch.int32)) and torch.equal(ix.assignments, km.assignments)
    assert ix.rows == N == len(ix.pq) and torch.equal(ix.labels, lab) and not ix.stale
    nn, cen, a = _np(M.l2_normalize_rows(x)), _np(ix.centroids), _np(ix.assignments)
    cb, dist = V.train(nn, a, cen, Mq, 3, cluster.seeded_rows(N, 256, 1))
    _assert_bits(ix.codebooks, cb, "codebooks")
    codes = V.encode(nn, a, cen, cb)
    assert (_np(ix.codes) == codes).all() and (_np(ix.list_codes) == codes[_np(ix.order)]).all()
    assert dist[-1] < dist[0]
    _assert_bits(ix.reconstruct(), V.reconstruct(codes, a, cen, cb), "reconstruct")
    # train_rows: the rows seeded_rows picks, in that order, then the start of the loop among those
    half = Index.build(x, Mq, nlist, iters=4, pq_iters=3, seed=1, train_rows=512)
    tp = cluster.seeded_rows(N, 512, 1)
    cb2, _ = R.lloyd(V.residuals(nn, a, cen)[tp], Mq, 3, cluster.seeded_rows(512, 256, 1))
    _assert_bits(half.codebooks, cb2, "train_rows codebooks")
    assert not np.array_equal(cb, cb2) and (_np(half.codes) == V.encode(nn, a, cen, cb2)).all()
    # a Gallery brings its normalised rows and its labels
    gal = Gallery(D, DEV).add(x, lab)
    ig = Index.build(gal, Mq, nlist, iters=4, pq_iters=3, seed=1)
    cen, a = _np(ig.centroids), _np(ig.assignments)
    cbg, _ = V.train(_np(gal.data), a, cen, Mq, 3, cluster.seeded_rows(N, 256, 1))
    _assert_bits(ig.codebooks, cbg, "Gallery codebooks")
    assert (_np(ig.codes) == V.encode(_np(gal.data), a, cen, cbg)).all() and torch.equal(ig.labels, lab)


# ---- 9. add
def test_add_in_pieces_equals_add_at_once():
    D, Mq = 64, 16
    m = _model(D, Mq)
    x, q, cen, cb = m["x"], m["q"], m["cen"], m["cb"]
    lab = _dev(m["lab"])
    whole = Index(cen, cb).add(x, lab)                                 # assign_clusters decides the lists
    assert torch.equal(whole.assignments, M.assign_clusters(x, cen)[0])
    parts = Index(cen, cb).add(x[:1700], lab[:1700])
    cap0 = parts.pq._codes.shape[0]
    assert parts.add(x[1700:], lab[1700:]) is parts and parts.rows == G == len(parts.pq) and parts.pq._codes.shape[0] > cap0
    assert parts.add(x[:0]) is parts and parts.rows == G
    for name in ("codes", "assignments", "offsets", "order", "counts", "list_codes", "labels"):
        assert torch.equal(getattr(parts, name), getattr(whole, name)), name
    for k in (3, 150):
        _same(parts.search(q, k, nprobe=3), whole.search(q, k, nprobe=3), f"k={k}")
    a = _np(whole.assignments)
    _assert_bits(whole.reconstruct(), V.reconstruct(_np(whole.codes), a, _np(cen), _np(cb)), "reconstruct")
    assert whole.nbytes == NLIST * D * 4 + 8 * (G + NLIST + 1 + G + NLIST) + G * Mq + whole.pq.nbytes
    with pytest.raises(MI355Error, match=r"an assignment outside \[0, nlist=6\)"):
        Index(cen, cb).add(x[:10], assignments=torch.full((10,), 6, device=DEV))
    empty = Index(cen, cb)
    assert empty.rows == 0 and empty.list_codes.shape == (0, Mq)
    with pytest.raises(MI355Error, match="k out of range"):
        empty.search(q, 1, nprobe=1)


# ---- 10. quality
def test_residual_codes_recall_more_than_plain_codes():
    rows = R.clustered_rows(4096 + 64, 64, 32, 0.3, 0)
    q, gal = _dev(rows[:64]), Gallery(64, DEV).add(_dev(rows[64:]))
    plain = pq.PQGallery.from_gallery(gal, 16)
    ix = Index.build(gal, 16, 32)
    mine, theirs = ix.recall(q, 10, nprobe=32, exact=gal)[0], plain.recall(q, 10, gal)[0]

    def err(recon):
        d = (gal.data - recon).double()
        return float((d * d).sum(dim=1).mean())

    e_mine, e_theirs = err(ix.reconstruct()), err(plain.reconstruct())
    print(f"recall@10: plain {theirs:.3f}, residual {mine:.3f}; quantisation error: plain {e_theirs:.5f}, residual {e_mine:.5f} "
          f"(ratio {e_mine / e_theirs:.3f})")
    assert mine >= theirs
    assert e_mine < 0.75 * e_theirs


# ---- 11. side streams
SD, SM = 64, 16


def _stream_parts():
    cb = (_randn((SM, 256, SD // SM), 901) / 8.0).contiguous()
    cen = M.l2_normalize_rows(_randn((6, SD), 905))
    return cb, cen, _randn((3000, SD), 902)


def _stream_index():
    cb, cen, x = _stream_parts()
    return Index(cen, cb).add(x, torch.arange(3000, device=DEV) % 7), x


def _pair(shape):
    return {"x": _randn(shape, 903)}, {"x": _randn(shape, 904)}


def _make_build(dev):
    def op(i):
        ix = Index.build(i["x"], SM, 6, iters=2, pq_iters=2)
        return ix.centroids, ix.assignments, ix.offsets, ix.order, ix.codebooks, ix.codes, ix.list_codes
    return (op,) + _pair((1500, SD))


def _make_add(dev):
    cb, cen, x = _stream_parts()

    def op(i):
        ix = Index(cen, cb).add(x[:1000]).add(i["x"])
        return ix.assignments, ix.offsets, ix.order, ix.codes, ix.list_codes
    return (op,) + _pair((700, SD))


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


def _make_coarse(dev):
    ix, _ = _stream_index()
    probes = (torch.arange(37 * 3, device=dev).view(37, 3) * 5) % 6
    return (lambda i: ix.coarse(i["x"], probes),) + _pair((37, SD))


STREAM_CASES = [H.Case("ResidualIVFPQIndex.build", ("ResidualIVFPQIndex.build",), _make_build, syncs=True),
                H.Case("ResidualIVFPQIndex.add", ("ResidualIVFPQIndex.add",), _make_add, syncs=True),
                H.Case("ResidualIVFPQIndex.search", ("ResidualIVFPQIndex.search",), _make_search, syncs=True),
                H.Case("ResidualIVFPQIndex.search filtered", ("ResidualIVFPQIndex.search",), _make_filtered, syncs=True),
                H.Case("ResidualIVFPQIndex.search refined", ("ResidualIVFPQIndex.search",), _make_refined, syncs=True),
                H.Case("ResidualIVFPQIndex.coarse", ("ResidualIVFPQIndex.coarse",), _make_coarse, syncs=False)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
