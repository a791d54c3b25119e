"""IVF search over an int8 gallery on the GPU against the NumPy model of the contract (ivf_i8_ref.py) BIT FOR BIT: values as
their 32-bit patterns, indices as they are.  A score is the int8 score of the gallery's own row (the codes and scales are read
back: the quantiser is tested in test_gallery_i8_gpu.py), the rows a query sees are those of its probed lists, and the
selection is the library's.  Eight hand-made lists whose lengths sit on the edges of the scan's chunk of 64 rows, scattered
over the gallery by a seeded permutation.  Three widths: D = 70 (ld 128, 8 chunks of 16 bytes: most lanes idle), 1536 (96
chunks: a half-filled second lane trip) and 4100 (ld 4224, 264 chunks: the four-loads-in-flight loop takes a second trip, and a
group shrinks from 8 queries to 7)."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import ivf_i8_ref as R
import ivf_ref as I
import gallery_i8_ref as R8
import stream_harness as H
from imageretrievalresearch_amd import Gallery, IVFIndex, Int8Gallery, MI355Error, _lib, ivf_i8
from imageretrievalresearch_amd import rank as _rank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [0, 1, 3, 63, 64, 65, 129, 300]
NLIST, G, NQ = len(LENGTHS), sum(LENGTHS), 200
E, ONE, THREE, L63, L64, L65, L129, L300 = range(NLIST)
DIMS = (70, 1536, 4100)
KS = (1, 3, 8, 9, 150)
TWINS = (17, 411)                                   # two identical rows, put into different lists


def _randn(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_bits(got, want, what=""):
    """float32 arrays equal as 32-bit patterns; a NaN equals any NaN."""
    got = np.ascontiguousarray(_np(got) if torch.is_tensor(got) else got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.uint32)[~gn] == want.view(np.uint32)[~wn]).all(), what


def _same(a, b, what=""):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), what


def _assignments():
    a = np.empty(G, np.int64)
    a[np.random.RandomState(5).permutation(G)] = np.repeat(np.arange(NLIST), LENGTHS)
    i, j = TWINS
    if a[i] == a[j]:                                # the twins in different lists: swap one with a row of another list
        o = int(np.flatnonzero(a != a[i])[0])
        a[j], a[o] = a[o], a[j]
    return a


_models = {}


def _model(D):
    """Seeded rows and queries of one width, the gallery and the index over the hand-made lists on the GPU, and the model's
    score of every (query, row) pair from the codes read back.  Made once per width and left unchanged."""
    if D not in _models:
        x, q = _randn((G, D), 100 + D), _randn((NQ, D), 200 + D)
        x[TWINS[1]] = x[TWINS[0]]
        q[0] = x[TWINS[0]] + 0.01 * q[0]            # a query whose two best rows are the twins
        lab = torch.randint(0, 4, (G,), generator=torch.Generator().manual_seed(D)).to(DEV)
        gal = Int8Gallery(D, DEV).add(x, lab)
        assign = _assignments()
        ix = ivf_i8.Int8IVFIndex(gal, _randn((NLIST, D), 400 + D), _dev(assign))
        offsets, order = I.lists_of(assign, NLIST)
        assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
        s = R.pair_scores(_np(M.l2_normalize_rows(q)), _np(gal.codes), _np(gal.scales))
        _models[D] = dict(x=x, q=q, gal=gal, ix=ix, s=s, offsets=offsets, order=order, lab=_np(lab), assign=assign, top={})
    return _models[D]


def _rot(lists, n=NQ):
    lists = np.asarray(lists, np.int64)
    return np.stack([np.roll(lists, -qi) for qi in range(n)])


PROBES = {
    "only the empty list": np.full((NQ, 1), E, np.int64),
    "fewer rows than k": _rot([E, ONE, THREE]),
    "nprobe = 1": (np.arange(NQ, dtype=np.int64) % NLIST)[:, None],              # 25 queries per list: groups of 8, 8, 8, 1
    "chunk edges": np.tile(np.array([L63, L65, ONE, L64], np.int64), (NQ, 1)),
    "nprobe = nlist": _rot(np.random.RandomState(6).permutation(NLIST)),
    "queries of different lengths": np.array([[[E, ONE, THREE], [L63, L64, L65], [L129, E, L300], [L300, L65, L63], [THREE, L64, ONE]][qi % 5]
                                              for qi in range(NQ)], np.int64),
}


def _want(m, name):
    """The model's top-150 of every query over its probed rows, once per probe set: a smaller k or Q is a prefix."""
    if name not in m["top"]:
        m["top"][name] = R.search(m["s"], m["offsets"], m["order"], PROBES[name], max(KS))
    return m["top"][name]


def _check_slab(m, q, probes, cap, what, ok=None, idx_offset=0, filt=None, rows=None):
    cv, ci = m["ix"]._scan(q, _dev(probes), cap, idx_offset, filt)
    s = m["s"] if rows is None else m["s"][rows]
    wv, wi = R.slab(s, m["offsets"], m["order"], probes, cap, ok, idx_offset)
    assert (_np(ci) == wi).all(), what
    _assert_bits(cv, wv, what)


# ---- 1. slab and search against the model
@pytest.mark.parametrize("D", DIMS)
def test_slab_and_search_equal_the_model(D):
    m = _model(D)
    ix = m["ix"]
    for name, probes in PROBES.items():
        wv, wi = _want(m, name)
        if name == "fewer rows than k":
            assert (wi[:, :4] >= 0).all() and (wi[:, 4:] == -1).all()
        if name == "only the empty list":
            assert (wi == -1).all() and np.isinf(wv).all()
        longest = max(sum(LENGTHS[l] for l in p) for p in probes)
        for Q in (1, 3, NQ):
            _check_slab(m, m["q"][:Q], probes[:Q], max(longest, 1) + 5, f"D={D} {name} Q={Q} slab", rows=slice(0, Q))
            p = _dev(probes[:Q])
            for k in KS:
                v, i = ix.search(m["q"][:Q], k, probes=p)
                what = f"D={D} {name} Q={Q} k={k}"
                assert (_np(i) == wi[:Q, :k]).all(), what
                _assert_bits(v, wv[:Q, :k], what)


# ---- 2. group edges
@pytest.mark.parametrize("D", DIMS)
def test_group_edges(D):
    """Single lists probed by exactly 1, 7, 8, 9 and 17 queries: whole groups of 8 (of 7 at D = 4100) and a remainder of 1."""
    m = _model(D)
    lists = np.concatenate([np.full(n, l) for l, n in ((L300, 1), (L129, 7), (L65, 8), (L64, 9), (L63, 17))]).astype(np.int64)
    lists = lists[np.random.RandomState(9).permutation(lists.size)]              # the queries of a list are not neighbours
    assert sorted(np.bincount(lists)[[L300, L129, L65, L64, L63]]) == [1, 7, 8, 9, 17]
    Q = lists.size
    _check_slab(m, m["q"][:Q], lists[:, None], 300, f"D={D}", rows=slice(0, Q))
    v, i = m["ix"].search(m["q"][:Q], 9, probes=_dev(lists[:, None]))
    wv, wi = R.search(m["s"][:Q], m["offsets"], m["order"], lists[:, None], 9)
    assert (_np(i) == wi).all()
    _assert_bits(v, wv)


# ---- 3. every list probed = the exhaustive search
@pytest.mark.parametrize("D", DIMS)
def test_every_list_probed_equals_the_exhaustive_search(D):
    m = _model(D)
    ix, gal, q = m["ix"], m["gal"], m["q"]
    assert m["assign"][TWINS[0]] != m["assign"][TWINS[1]]
    for Q in (1, 3, 5, 9, NQ):                      # the exhaustive side: GEMV up to 4 queries, GEMM tiles above
        for k in (3, 150):
            got, want = ix.search(q[:Q], k, nprobe=NLIST), gal.search(q[:Q], k)
            _same(got, want, f"D={D} Q={Q} k={k}")
            assert _np(got[1])[0, :2].tolist() == list(TWINS)                    # an exact tie across lists: the lower row first
            assert int(got[0][0, 0].view(torch.int32)) == int(got[0][0, 1].view(torch.int32))
    wv, wi = R8.topk(m["s"], 150)
    v, i = ix.search(q, 150, nprobe=NLIST)
    assert (_np(i) == wi).all()
    _assert_bits(v, wv)
    _same(ix.search(q, 8, nprobe=NLIST, idx_offset=7000), gal.search(q, 8, idx_offset=7000), "idx_offset")


# ---- 4. what the bits do not depend on
@pytest.mark.parametrize("D", (70, 4100))
def test_bits_do_not_depend_on_batch_nprobe_block_or_group(D):
    m = _model(D)
    ix, q = m["ix"], m["q"]
    probes = PROBES["queries of different lengths"]
    many = ix.search(q, 8, probes=_dev(probes))
    for qi in (0, 7, 199):                          # a query alone against inside 200
        one = ix.search(q[qi:qi + 1], 8, probes=_dev(probes[qi:qi + 1]))
        _same(one, (many[0][qi:qi + 1].contiguous(), many[1][qi:qi + 1].contiguous()), f"query {qi} alone")
    for block in (1, 7, 64):
        _same(ix.search(q, 8, probes=_dev(probes), block=block), many, f"block={block}")
    perm = np.random.RandomState(11).permutation(NQ)                              # other queries share its group
    shuffled = ix.search(q[_dev(perm)], 8, probes=_dev(probes[perm]))
    _same(shuffled, (many[0][_dev(perm)], many[1][_dev(perm)]), "group mates")
    # nprobe: the score of a (query, row) pair in the slab of two lists and in the slab of all lists
    few, all_ = PROBES["nprobe = nlist"][:, :2], PROBES["nprobe = nlist"]
    fv, fi = (_np(t) for t in ix._scan(q, _dev(few), G, 0, None))
    av, ai = (_np(t) for t in ix._scan(q, _dev(all_), G, 0, None))
    for qi in range(0, NQ, 13):
        full = dict(zip(ai[qi].tolist(), av[qi].view(np.uint32).tolist()))
        n = int((fi[qi] != R.NO_CAND).sum())
        assert n == sum(LENGTHS[l] for l in few[qi])
        assert all(full[r] == b for r, b in zip(fi[qi, :n].tolist(), fv[qi, :n].view(np.uint32).tolist()))


# ---- 5. special rows and queries
def test_nan_and_zero_rows_and_a_nan_query():
    D, n = 70, 130
    x, q = _randn((n, D), 31), _randn((9, D), 32)
    x[40, 3] = float("nan")
    x[90] = 0.0
    q[4, 5] = float("nan")
    gal = Int8Gallery(D, DEV).add(x)
    assign = np.arange(n) % 3
    ix = ivf_i8.Int8IVFIndex(gal, _randn((3, D), 33), _dev(assign))
    offsets, order = I.lists_of(assign, 3)
    s = R.pair_scores(_np(M.l2_normalize_rows(q)), _np(gal.codes), _np(gal.scales))
    assert np.isnan(s[:, 40]).all() and (s[[0, 1, 2, 3, 5, 6, 7, 8], 90] == 0).all() and np.isnan(s[4]).all()
    probes = _rot([1, 0, 2], 9)
    for k in (1, 8, 100):
        v, i = ix.search(q, k, probes=_dev(probes))
        wv, wi = R.search(s, offsets, order, probes, k)
        assert (_np(i) == wi).all()
        _assert_bits(v, wv)
        _same((v, i), gal.search(q, k), f"k={k}")                                 # the NaN query: the exhaustive search's order
        finite = [0, 1, 2, 3, 5, 6, 7, 8]
        assert (_np(i)[finite, 0] == 40).all() and bool(torch.isnan(v[:, 0]).all())   # the NaN row ranks first, with score NaN
        assert bool(torch.isnan(v[4]).all()) and _np(i)[4].tolist() == list(range(k))  # the NaN query: every score NaN, row order
    cv, ci = ix._scan(q, _dev(probes), n, 0, None)
    where = _np(ci) == 90
    assert where.sum() == 9 and (_np(cv)[where][[0, 1, 2, 3, 5, 6, 7, 8]] == 0).all()
    # a list of one query holding only the zero and the NaN row
    two = ivf_i8.Int8IVFIndex(gal, _randn((2, D), 34), _dev(np.where(np.isin(np.arange(n), (40, 90)), 0, 1)))
    v, i = two.search(q[:1], 2, probes=_dev(np.zeros((1, 1), np.int64)))
    assert _np(i).tolist() == [[40, 90]] and bool(torch.isnan(v[0, 0])) and float(v[0, 1]) == 0.0


# ---- 6. filters and pads
@pytest.mark.parametrize("D", (70, 1536))
def test_filters_and_pads(D):
    m = _model(D)
    ix, off = m["ix"], 5000
    probes = PROBES["queries of different lengths"]
    ql = np.arange(NQ) % 4
    best = R.search(m["s"], m["offsets"], m["order"], probes, 1)[1][:, 0]
    ex = np.where(np.arange(NQ) % 3 == 1, -1, best + off)                        # two thirds leave their best probed row out
    for label_filter in ("same", "different", None):
        ok = I.eligible(G, NQ, ql, m["lab"], label_filter, ex, off)
        kw = dict(idx_offset=off, query_labels=_dev(ql), label_filter=label_filter, exclude=_dev(ex))
        for k in (3, 9, 150):
            wv, wi = R.search(m["s"], m["offsets"], m["order"], probes, k, ok, off)
            for Q, block in ((1, None), (NQ, None), (NQ, 7)):                     # 7: 29 trips, each with its own queries' filter
                v, i = ix.search(m["q"][:Q], k, probes=_dev(probes[:Q]), block=block,
                                 **{n: (a[:Q] if torch.is_tensor(a) else a) for n, a in kw.items()})
                what = f"Q={Q} block={block} k={k} {label_filter}"
                assert (_np(i) == wi[:Q]).all(), what
                _assert_bits(v, wv[:Q], what)
        gl = None if label_filter is None else _dev(m["lab"])
        filt = _rank._rank_filter(NQ, G, torch.device(DEV), _dev(ql), gl, label_filter, _dev(ex))
        _check_slab(m, m["q"], probes, 500, f"slab {label_filter}", ok, off, filt)
    # fewer than k eligible probed rows: the tail is (-inf, -1)
    short = PROBES["fewer rows than k"]
    ok = I.eligible(G, NQ, ql, m["lab"], "same")
    v, i = ix.search(m["q"], 9, probes=_dev(short), query_labels=_dev(ql), label_filter="same")
    wv, wi = R.search(m["s"], m["offsets"], m["order"], short, 9, ok)
    assert (_np(i) == wi).all() and (wi[:, 4:] == -1).all() and np.isneginf(_np(v)[wi == -1]).all()
    _assert_bits(v, wv)
    with pytest.raises(MI355Error):                                               # no gallery labels
        ivf_i8.Int8IVFIndex(Int8Gallery(D, DEV).add(m["x"]), ix.centroids, ix.assignments) \
            .search(m["q"], 3, 2, query_labels=_dev(ql), label_filter="same")


# ---- 7. refine
def _exact_dots(exact, q):
    """Every pair's fp32 dot from the routine the refinement shares: one IVF list that holds every row (its slab is in row order)."""
    n = len(exact)
    one = IVFIndex(exact, M.l2_normalize_rows(exact.data[:1].float()), torch.zeros(n, dtype=torch.int64, device=DEV))
    cv, ci = one._scan(q, torch.zeros((q.shape[0], 1), dtype=torch.int64, device=DEV), n, 0, None)
    assert (_np(ci) == np.arange(n)[None, :]).all()
    return _np(cv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", (70, 1536))
def test_refine_rescoring(D, dtype):
    m = _model(D)
    ix, gal, q = m["ix"], m["gal"], m["q"]
    exact = Gallery(D, DEV, dtype=dtype).add(m["x"])
    dots32 = _exact_dots(exact, q)
    for name, k, short in (("queries of different lengths", 3, 20), ("chunk edges", 8, 100), ("nprobe = nlist", 20, 150),
                           ("fewer rows than k", 3, 50)):
        p = _dev(PROBES[name])
        si = _np(ix.search(q, short, probes=p)[1])                                # the unrefined shortlist
        assert (si == _want(m, name)[1][:, :short]).all()
        v, i = ix.search(q, k, probes=p, refine=exact, shortlist=short)
        wv, wi = R.refined(si, dots32, k)
        what = f"{name} k={k} shortlist={short}"
        assert (_np(i) == wi).all(), what
        _assert_bits(v, wv, what)
    for k, short, off in ((3, 100, 0), (8, 64, 900), (150, 1024 if G >= 1024 else G, 0)):   # the gallery's own search
        si = _np(gal.search(q, short, off)[1])
        v, i = gal.search(q, k, off, refine=exact, shortlist=short)
        wv, wi = R.refined(si, dots32, k, off)
        assert (_np(i) == wi).all(), (k, short)
        _assert_bits(v, wv, f"gallery k={k}")
        _same(ix.search(q, k, nprobe=NLIST, idx_offset=off, refine=exact, shortlist=short), (v, i), "every list, refined")
    v, i = gal.search(q, 3, refine=exact)                                         # the default shortlist: min(max(10 k, 100), 1024, rows)
    _same(gal.search(q, 3, refine=exact, shortlist=100), (v, i))
    _same(ix.search(q, 3, nprobe=NLIST, refine=exact), (v, i))
    ql = torch.arange(NQ, device=DEV) % 4
    _same(gal.search(q, 3, query_labels=ql, label_filter="same", refine=exact, shortlist=G),
          ix.search(q, 3, nprobe=NLIST, query_labels=ql, label_filter="same", refine=exact, shortlist=G), "filtered, refined")
    _same(gal.search(q, 5), _rank._topk(q, gal._resident(), 5, gal.eps))        # without them nothing changes


# ---- 8. from_gallery and recall
def test_from_gallery_lists_and_recall():
    D = 70
    m = _model(D)
    q = m["q"][:40]
    g = Gallery(D, DEV).add(m["x"], _dev(m["lab"]))
    ix = ivf_i8.Int8IVFIndex.from_gallery(g, 6, iters=3, seed=2)
    fp = g.ivf(6, iters=3, seed=2)
    for name in ("centroids", "assignments", "offsets", "order", "counts"):
        assert torch.equal(getattr(ix, name), getattr(fp, name)), name
    assert torch.equal(ix.i8.codes, m["gal"].codes) and torch.equal(ix.i8.labels, g.labels) and not ix.stale
    assert torch.equal(ix.probe(q, 2), fp.probe(q, 2))
    assert ix.nbytes == 6 * D * 4 + 8 * (G + 7 + G + 6)
    built = ix.i8.ivf(g, 6, iters=3, seed=2)                                      # the convenience: the same k-means, cached
    assert torch.equal(built.assignments, ix.assignments) and ix.i8.ivf(g, 6, iters=3, seed=2) is built
    offsets, order = _np(ix.offsets), _np(ix.order)
    for k, nprobe in ((3, 1), (10, 2)):
        probes = _np(ix.probe(q, nprobe))
        got = R.search(m["s"][:40], offsets, order, probes, k)[1]
        for exact, want in ((None, R8.topk(m["s"][:40], k)[1]), (g, _np(g.search(q, k)[1]))):
            hits = np.array([np.isin(want[qi], got[qi]).sum() for qi in range(40)])
            mean, per_q = ix.recall(q, k, nprobe, exact=exact)
            print(f"recall@{k} nprobe={nprobe} against {'the int8 search' if exact is None else 'the fp32 search'}: {mean:.3f}")
            # the library divides on the GPU, where x / k may be x * (1 / k): the counts are compared as integers
            assert (np.rint(_np(per_q) * k) == hits).all() and np.abs(_np(per_q) - hits / float(k)).max() < 1e-12
            assert abs(mean - float(hits.mean()) / k) < 1e-12
    mean, _ = ix.recall(q, 3, 6)
    assert mean == 1.0                                                            # every list probed: nothing lost to the lists


# ---- 9. add and staleness
def test_add_and_staleness():
    D = 70
    m = _model(D)
    x, q = m["x"], m["q"]
    lab = _dev(m["lab"])
    gal = Int8Gallery(D, DEV).add(x[:400], lab[:400])
    ix = ivf_i8.Int8IVFIndex.build(gal, x[:400], 5, iters=2)
    old = ix.assignments.clone()
    assert ix.add(x[400:], lab[400:]) is ix and not ix.stale and len(gal) == G == ix.rows
    assert torch.equal(ix.assignments[:400], old)
    assert torch.equal(ix.assignments[400:], M.assign_clusters(x[400:], ix.centroids)[0])
    whole = ivf_i8.Int8IVFIndex(m["gal"], ix.centroids, ix.assignments)          # built over all rows, the same centroids
    for name in ("offsets", "order", "counts"):
        assert torch.equal(getattr(ix, name), getattr(whole, name)), name
    assert torch.equal(gal.codes, m["gal"].codes) and torch.equal(gal.scales, m["gal"].scales)
    ql = torch.arange(NQ, device=DEV) % 4
    for k in (3, 150):
        _same(ix.search(q, k, nprobe=2), whole.search(q, k, nprobe=2), f"k={k}")
        _same(ix.search(q, k, nprobe=5), gal.search(q, k), f"k={k} every list")
    _same(ix.search(q, 8, nprobe=5, query_labels=ql, label_filter="same"), gal.search(q, 8, query_labels=ql, label_filter="same"))
    assert ix.add(x[:0]) is ix and ix.rows == G                                   # nothing to add
    gal.add(x[:1])                                                                # behind the index's back
    assert ix.stale
    with pytest.raises(MI355Error, match="stale: it lists 625 rows but the Int8Gallery holds 626 "
                                         r"\(add rows through index.add, or build the index again\)"):
        ix.search(q, 3, nprobe=2)
    with pytest.raises(MI355Error, match="stale"):
        ix.add(x[:1])


# ---- 10. errors found on the device
def test_bad_probes_and_a_short_cap_are_argument_errors():
    """A list id out of range and a cap below a query's probed rows raise the fp32 entry's messages; the slab sits between
    guard words that stay as they were."""
    D = 70
    m = _model(D)
    ix, gal, L = m["ix"], m["gal"], _lib.lib()
    Q, guard = 5, 256

    def scan(probes, cap):
        p = _dev(np.asarray(probes, np.int64))
        val = torch.full((Q * cap + 2 * guard,), 7.0, dtype=torch.float32, device=DEV)
        idx = torch.full((Q * cap + 2 * guard,), 7, dtype=torch.int64, device=DEV)
        ws = torch.empty(L.mi355_ivf_scan_i8_workspace_bytes(Q, p.shape[1], NLIST, D, cap), dtype=torch.uint8, device=DEV)
        rc = L.mi355_ivf_scan_i8(m["q"].data_ptr(), Q, D, gal.eps, gal._codes.data_ptr(), gal._scales.data_ptr(), gal._ld, G,
                                 ix.offsets.data_ptr(), ix.order.data_ptr(), NLIST, p.data_ptr(), p.shape[1], cap, 0, None,
                                 val[guard:].data_ptr(), idx[guard:].data_ptr(), ws.data_ptr(), ws.numel(),
                                 _lib.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        for t in (val, idx):
            assert bool((t[:guard] == 7).all()) and bool((t[guard + Q * cap:] == 7).all())
        return rc, L.mi355_last_error()

    good = np.tile(np.array([L63, L65], np.int64), (Q, 1))
    assert scan(good, 128)[0] == 0
    for bad_id in (NLIST, -1, 1 << 40):
        bad = good.copy()
        bad[3, 1] = bad_id
        rc, msg = scan(bad, 128)
        assert rc != 0 and b"ivf_scan_i8: a list id outside [0, nlist=8), an order entry outside [0, G=625)" in msg, msg
    rc, msg = scan(good, 127)                                                     # 63 + 65 rows
    assert rc != 0 and b"ivf_scan_i8: a query's probed lists hold more than cap=127 rows" in msg, msg
    rc, msg = scan(np.tile(np.array([L300, L129], np.int64), (Q, 1)), 70)         # a whole chunk past the cap
    assert rc != 0 and b"more than cap=70 rows" in msg, msg
    with pytest.raises(MI355Error, match=r"a list id outside \[0, nlist=8\)"):
        ix.search(m["q"][:Q], 3, probes=_dev(np.full((Q, 1), NLIST, np.int64)))


# ---- 11. side streams
SD = 70


def _stream_index(dev):
    x = _randn((1500, SD), 902)
    gal = Int8Gallery(SD, dev).add(x, torch.arange(1500, device=dev) % 7)
    return ivf_i8.Int8IVFIndex(gal, _randn((6, SD), 905), torch.arange(1500, device=dev) % 6), x


def _pair(shape):
    return {"x": _randn(shape, 903)}, {"x": _randn(shape, 904)}


def _make_search(dev):
    ix, _ = _stream_index(dev)
    ql, ex = torch.arange(37, device=dev) % 7, torch.arange(37, device=dev) * 5
    return (lambda i: (ix.search(i["x"], 3, 2), ix.search(i["x"], 150, 3, block=16), ix.search(i["x"], 8, nprobe=6),
                       ix.search(i["x"], 8, 3, query_labels=ql, label_filter="different", exclude=ex)),) + _pair((37, SD))


def _make_refined(dev):
    ix, x = _stream_index(dev)
    f32, f16 = Gallery(SD, dev).add(x), Gallery(SD, dev, dtype=torch.float16).add(x)
    return (lambda i: (ix.search(i["x"], 5, 3, refine=f32), ix.search(i["x"], 5, 3, refine=f16, shortlist=64),
                       ix.i8.search(i["x"], 5, refine=f32), ix.i8.search(i["x"], 5, refine=f16, shortlist=64)),) + _pair((37, SD))


def _make_add(dev):
    x = _randn((1000, SD), 902)
    cen = _randn((6, SD), 905)
    a = torch.arange(1000, device=dev) % 6

    def op(i):
        ix = ivf_i8.Int8IVFIndex(Int8Gallery(SD, dev).add(x), cen, a).add(i["x"])
        return ix.assignments, ix.offsets, ix.order, ix.i8.codes, ix.i8.scales
    return (op,) + _pair((700, SD))


def _make_build(dev):
    def op(i):
        ix = Int8Gallery(SD, dev).add(i["x"]).ivf(i["x"], 6, iters=2)
        return ix.centroids, ix.assignments, ix.offsets, ix.order
    return (op,) + _pair((1500, SD))


STREAM_CASES = [H.Case("Int8IVFIndex.build", ("Int8IVFIndex.build", "Int8Gallery.ivf"), _make_build, syncs=True),
                H.Case("Int8IVFIndex.search", ("Int8IVFIndex.search",), _make_search, syncs=True),
                H.Case("Int8IVFIndex.search refined", ("Int8IVFIndex.search", "Int8Gallery.search"), _make_refined, syncs=True),
                H.Case("Int8IVFIndex.add", ("Int8IVFIndex.add",), _make_add, syncs=True)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
