"""The IVF search on the GPU against the float64 reference (tests/ivf_ref.py).  The indexes are built from hand-made
assignments, so the test controls the lists: an empty list, a list of one row, lengths on either side of a group of 4 queries
and of the 64-row chunk, and one list that holds most of the rows (several chunks).  fp32 and fp16 galleries."""
import functools

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import ivf_ref as ref
from helpers import SCORE_TOL, assert_topk_matches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16}
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 295]          # the last: most of the 500 rows, longer than a chunk
NLIST, G = len(LENGTHS), sum(LENGTHS)
DIMS = [1, 7, 64, 70, 1536]
QS = [1, 3, 4, 5, 9, 67]
KS = [1, 3, 8, 9, 150]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).numpy()


@functools.lru_cache(maxsize=None)
def _assign():
    a = np.repeat(np.arange(NLIST), LENGTHS)
    return a[np.random.default_rng(7).permutation(G)].astype(np.int64)      # the lists' rows lie scattered


@functools.lru_cache(maxsize=None)
def _raw(seed, n, D):
    return (np.random.default_rng(seed).standard_normal((n, D)) * 1.3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _index(kind, D):
    """(index, the float64 rows as stored, offsets, order): the 500-row gallery under the hand-made lists."""
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(_raw(1, G, D)).to(DEV),
                                                  labels=torch.from_numpy(np.random.default_rng(3).integers(0, 4, G)).to(DEV))
    cent = torch.from_numpy(_raw(2, NLIST, D)).to(DEV)
    ix = M.IVFIndex(g, cent, torch.from_numpy(_assign()).to(DEV))
    offsets, order = ref.lists_of(_assign(), NLIST)
    assert (ix.offsets.cpu().numpy() == offsets).all() and (ix.order.cpu().numpy() == order).all()
    return ix, g.data.float().cpu().numpy().astype(np.float64), offsets, order


def _probes(Q, nprobe, seed=0):
    """Distinct lists per query; query 0 starts at the empty list, query 1 (if any) at the one-row list, and the low ids make
    many queries share lists."""
    rng = np.random.default_rng(100 * Q + nprobe + seed)
    p = np.stack([rng.permutation(NLIST)[:nprobe] for _ in range(Q)]).astype(np.int64)
    for q, first in ((0, 0), (1, 1)):
        if q < Q:
            rest = [l for l in p[q] if l != first][: nprobe - 1]
            p[q] = np.array([first] + rest, np.int64)
    return p


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kind", list(DTYPES))
def test_scan_and_search_match_float64(kind, D):
    ix, rows, offsets, order = _index(kind, D)
    worst = 0.0
    for Q in QS:
        x = _raw(10 + Q, Q, D)
        q = torch.from_numpy(x).to(DEV)
        for nprobe in (1, 2, NLIST):
            p = _probes(Q, nprobe)
            pt = torch.from_numpy(p).to(DEV)
            S = ref.restricted_scores(rows, x, offsets, order, p)
            # the candidate slab itself: the members of the probed lists, each once, in list order, then pads
            cap = int(ix._longest[nprobe])
            cv, ci = (t.cpu().numpy() for t in ix._scan(q, pt, cap, 0, None))
            for i in range(Q):
                want = ref.probed_rows(offsets, order, p[i])
                assert (ci[i, : want.size] == want).all(), (Q, nprobe, i)
                assert (ci[i, want.size:] >= ref.NO_CAND).all(), (Q, nprobe, i)
                if want.size:
                    worst = max(worst, float(np.abs(cv[i, : want.size] - S[i, want]).max()))
            assert worst <= SCORE_TOL
            for k in KS:
                v, i = ix.search(q, k, probes=pt)
                wv, wi, gap = ref.topk(S, k)
                assert_topk_matches(v.cpu().numpy(), i.cpu().numpy(), wv, wi, gap=gap, what=f"{kind} D={D} Q={Q} nprobe={nprobe} k={k}",
                                    scores_ref=S)
    print(f"{kind} D={D}: max |slab score - f64| {worst:.3e}")


def test_one_row_list_pads():
    ix, rows, offsets, order = _index("f32", 64)
    q = torch.from_numpy(_raw(5, 2, 64)).to(DEV)
    p = torch.tensor([[0], [1]], dtype=torch.int64, device=DEV)                  # the empty list, the one-row list
    v, i = ix.search(q, 3, probes=p)
    v, i = v.cpu().numpy(), i.cpu().numpy()
    assert (i[0] == -1).all() and np.isneginf(v[0]).all()
    assert i[1, 0] == order[offsets[1]] and (i[1, 1:] == -1).all() and np.isneginf(v[1, 1:]).all() and np.isfinite(v[1, 0])


@pytest.mark.parametrize("kind", list(DTYPES))
def test_probe_is_the_fp32_topk_of_the_centroids(kind):
    ix, *_ = _index(kind, 70)
    q = torch.from_numpy(_raw(21, 9, 70)).to(DEV)
    for nprobe in (1, 2, NLIST):
        assert (_bits(ix.probe(q, nprobe)) == _bits(M.cosine_topk(q, ix.centroids, nprobe)[1])).all()


@pytest.mark.parametrize("D", [70, 1536])
@pytest.mark.parametrize("kind", list(DTYPES))
def test_score_bits_do_not_depend_on_the_batch(kind, D):
    ix, *_ = _index(kind, D)
    Q, k = 9, 8
    q = torch.from_numpy(_raw(31, Q, D)).to(DEV)
    p = torch.from_numpy(_probes(Q, 2)).to(DEV)
    p[2:6] = p[2]                                                                 # four queries share both lists, in order
    v, i = ix.search(q, k, probes=p)
    for j in range(Q):
        v1, i1 = ix.search(q[j: j + 1], k, probes=p[j: j + 1])
        assert (_bits(v1[0]) == _bits(v[j])).all() and (_bits(i1[0]) == _bits(i[j])).all(), j
    v2, i2 = ix.search(q, k, probes=p, block=2)
    assert (_bits(v2) == _bits(v)).all() and (_bits(i2) == _bits(i)).all()
    # nprobe = 2 against every list: a row found by both has the same score bits
    va, ia = ix.search(q, k, nprobe=2)
    vb, ib = ix.search(q, G, nprobe=NLIST)                                        # every row of the gallery, ranked
    va, ia, vb, ib = _bits(va), ia.cpu().numpy(), _bits(vb), ib.cpu().numpy()
    common = 0
    for j in range(Q):
        where = {int(r): s for r, s in zip(ib[j], vb[j])}
        for r, s in zip(ia[j], va[j]):
            if r >= 0:
                assert where[int(r)] == s, (j, r)
                common += 1
    assert common > 0


@pytest.mark.parametrize("kind", list(DTYPES))
def test_every_list_probed_is_the_exact_search(kind):
    for D in (7, 1536):
        ix, rows, offsets, order = _index(kind, D)
        x = _raw(41, 9, D)
        S = ref.normalise(x) @ rows.T
        for k in (1, 9, 150):
            v, i = ix.search(torch.from_numpy(x).to(DEV), k, nprobe=NLIST)
            wv, wi, gap = ref.topk(S, k)
            assert_topk_matches(v.cpu().numpy(), i.cpu().numpy(), wv, wi, gap=gap, what=f"{kind} D={D} k={k}", scores_ref=S)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_filters(kind):
    D, Q, k = 64, 9, 9
    ix, rows, offsets, order = _index(kind, D)
    own = np.array([3, 17, 99, 250, 251, 300, 421, 498, 0], np.int64)            # the queries are gallery rows
    x = _raw(1, G, D)[own]
    q = torch.from_numpy(x).to(DEV)
    glab = ix.gallery.labels.cpu().numpy()
    qlab = glab[own]
    a = _assign()
    p = np.stack([np.concatenate([[a[r]], [l for l in (8, 5, 6) if l != a[r]][:1]]) for r in own]).astype(np.int64)   # own list first
    pt = torch.from_numpy(p).to(DEV)
    cases = [dict(exclude=own), dict(label_filter="same"), dict(label_filter="different"),
             dict(label_filter="different", exclude=own), dict(exclude=own + 1000, idx_offset=1000)]
    for c in cases:
        off = c.get("idx_offset", 0)
        S = ref.restricted_scores(rows, x, offsets, order, p, query_labels=qlab, gallery_labels=glab,
                                  label_filter=c.get("label_filter"), exclude=c.get("exclude"), idx_offset=off)
        kw = dict(idx_offset=off)
        if "exclude" in c:
            kw["exclude"] = torch.from_numpy(c["exclude"]).to(DEV)
        if "label_filter" in c:
            kw.update(label_filter=c["label_filter"], query_labels=torch.from_numpy(qlab).to(DEV))
        wv, wi, gap = ref.topk(S, k, off)
        whole = None
        for block in (None, 2, 4):            # one trip; five and three trips, the last ragged: every block its own queries' filter
            tv, ti = ix.search(q, k, probes=pt, block=block, **kw)
            v, i = tv.cpu().numpy(), ti.cpu().numpy()
            local = np.where(i >= 0, i - off, 0)
            assert (np.isfinite(np.take_along_axis(S, local, axis=1)) | (i < 0)).all(), (c, block)   # an ineligible row never appears
            if "exclude" in c:
                assert not (i == c["exclude"][:, None]).any(), (c, block)
            # assert_topk_matches looks scores up by the returned index: hand it local indices
            assert_topk_matches(v, np.where(i >= 0, i - off, -1), wv, np.where(wi >= 0, wi - off, -1), gap=gap,
                                what=f"{sorted(c)} block={block}", scores_ref=S)
            if whole is None:
                whole = _bits(tv), _bits(ti)
            assert (_bits(tv) == whole[0]).all() and (_bits(ti) == whole[1]).all(), (c, block)


def _planted():
    rng = np.random.default_rng(11)
    centres = np.eye(64, dtype=np.float32)[:8]
    lab = np.repeat(np.arange(8), 40)
    rows = (centres[lab] + 0.05 * rng.standard_normal((320, 64))).astype(np.float32)
    qlab = np.repeat(np.arange(8), 3)
    qs = (centres[qlab] + 0.05 * rng.standard_normal((24, 64))).astype(np.float32)
    return centres, lab, rows, qlab, qs


@pytest.mark.parametrize("kind", list(DTYPES))
def test_planted_clusters_need_one_probe(kind):
    centres, lab, x, qlab, qs = _planted()
    g = M.Gallery(64, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(x).to(DEV))
    rows = g.data.float().cpu().numpy().astype(np.float64)
    # float64 first: the planted structure is certified before the GPU result is looked at
    S = ref.normalise(qs) @ rows.T
    top5 = np.argsort(-S, axis=1, kind="stable")[:, :5]
    assert (lab[top5] == qlab[:, None]).all()
    srt = np.sort(S, axis=1)[:, ::-1]
    own_worst = np.array([S[q, lab == qlab[q]].min() for q in range(24)])
    other_best = np.array([S[q, lab != qlab[q]].max() for q in range(24)])
    assert (own_worst - other_best).min() > 0.5 and (srt[:, :5] - srt[:, 1:6]).min() > 1e-5
    assert ((ref.normalise(centres) @ rows.T).argmax(axis=0) == lab).all()
    ix = M.IVFIndex.build(g, 8, init=torch.from_numpy(centres).to(DEV))
    assert (ix.assignments.cpu().numpy() == lab).all()                           # the lists are the planted clusters
    offsets, order = ref.lists_of(lab, 8)
    assert (ix.offsets.cpu().numpy() == offsets).all() and (ix.order.cpu().numpy() == order).all()
    q = torch.from_numpy(qs).to(DEV)
    v, i = ix.search(q, 5, nprobe=1)
    ev, ei = g.search(q, 5)
    assert (i.cpu().numpy() == ei.cpu().numpy()).all() and (i.cpu().numpy() == top5).all()
    np.testing.assert_allclose(v.cpu().numpy(), ev.cpu().numpy(), rtol=0, atol=SCORE_TOL)
    mean, per = ix.recall(q, 5, 1)
    assert mean == 1.0 and per.shape == (24,) and bool((per == 1.0).all())


def test_update_and_cache():
    centres, lab, x, qlab, qs = _planted()
    g = M.Gallery(64, DEV).add(torch.from_numpy(x[:300]).to(DEV))
    ix = g.ivf(8, iters=3, seed=1)
    assert g.ivf(8, iters=3, seed=1) is ix and g.ivf(8, iters=3, seed=2) is not ix
    assert ix.nbytes == 8 * 64 * 4 + 8 * (300 + 9 + 300 + 8)
    g.add(torch.from_numpy(x[300:]).to(DEV))
    assert g._ivf == {} and ix.stale
    q = torch.from_numpy(x[300:]).to(DEV)
    with pytest.raises(M.MI355Error, match="stale"):
        ix.search(q, 1, nprobe=8)
    old = ix.assignments.clone()
    ix.update()
    assert not ix.stale and ix.rows == 320 and (ix.assignments[:300] == old).all()
    want = M.assign_clusters(g, ix.centroids)[0]
    assert (ix.assignments == want).all()                                        # the new rows went to their nearest list
    v, i = ix.search(q, 1, nprobe=8)
    assert (i[:, 0].cpu().numpy() == np.arange(300, 320)).all()                  # every new row finds itself
    assert g.ivf(8, iters=3, seed=1) is not ix
