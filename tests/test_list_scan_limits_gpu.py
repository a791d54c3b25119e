"""The list scans where their loops take a second trip: more IVF work items than the scan's grid has workgroups, more lists
than k_ivf_plan has threads, more queries than one workgroup of k_ivf_bases, more probes than one workgroup of k_ivfpq_coarse
(64) and than the threads that stage base[] and coarse[] (256 or 1024), long runs of empty lists under the cursor of the
IVF-PQ scans, and M = 128 with nprobe = 1024: the launch that asks for the dynamic LDS the header declares as the maximum.
The IVF scan is checked against float64 (tests/ivf_ref.py), the two IVF-PQ searches against their NumPy models bit for bit
(pq_ref.py, ivfrpq_ref.py).  Every case asserts the condition it is there for."""
import functools

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import ivf_ref as I
import ivfrpq_ref as V
import pq_ref as R
from helpers import SCORE_TOL, assert_topk_matches
from imageretrievalresearch_amd import _lib, ivfpq, ivfrpq, pq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16}
IVF_NQ, IVF_CHUNK = 4, 64                                            # queries of a group, rows of a work item (ivf.hip)
PLAN_THREADS, BASES_THREADS, COARSE_CHUNK = 1024, 256, 64           # k_ivf_plan, k_ivf_bases, k_ivfpq_coarse


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).numpy()


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raw(seed, n, D):
    return (np.random.default_rng(seed).standard_normal((n, D)) * 1.3).astype(np.float32)


def _assert_bits(got, want, what=""):
    """float32 arrays equal as int32 bit patterns; a NaN equals any NaN."""
    got, want = np.ascontiguousarray(_np(got), dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.int32)[~gn] == want.view(np.int32)[~wn]).all(), what


def _cdiv(a, b):
    return -(-a // b)


def _check_slab(ix, q, p, rows, x, offsets, order, what):
    """The candidate slab of ``_scan`` and the scores in it against float64; returns the reference's restricted scores."""
    S = I.restricted_scores(rows, x, offsets, order, p)
    cap = int(ix._longest[p.shape[1]])
    cv, ci = (_np(t) for t in ix._scan(q, _dev(p), cap, 0, None))
    worst = 0.0
    for i in range(p.shape[0]):
        want = I.probed_rows(offsets, order, p[i])
        assert (ci[i, : want.size] == want).all(), (what, i)
        assert (ci[i, want.size:] >= I.NO_CAND).all(), (what, i)
        if want.size:
            worst = max(worst, float(np.abs(cv[i, : want.size] - S[i, want]).max()))
    assert worst <= SCORE_TOL, (what, worst)
    return S


# ---- a. more work items than two passes of the scan's grid
@pytest.mark.parametrize("D", [64, 70])
@pytest.mark.parametrize("kind", list(DTYPES))
def test_ivf_scan_workgroups_take_several_items(kind, D):
    nlist, length, Q = 40, 65, 300
    G = nlist * length
    assign = np.repeat(np.arange(nlist), length)[np.random.default_rng(7).permutation(G)].astype(np.int64)
    glab = np.random.default_rng(3).integers(0, 4, G)
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(_dev(_raw(1, G, D)), labels=_dev(glab))
    ix = M.IVFIndex(g, _dev(_raw(2, nlist, D)), _dev(assign))
    offsets, order = I.lists_of(assign, nlist)
    assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
    rows = _np(g.data.float()).astype(np.float64)
    p = np.stack([np.roll(np.arange(nlist, dtype=np.int64), -qi) for qi in range(Q)])    # every list, each query its own rotation
    # the item table: per list cdiv(pairs, nq) groups x cdiv(rows, 64) chunks; the grid is 8 workgroups per CU
    pairs = np.bincount(p.reshape(-1), minlength=nlist)
    items = int(sum(_cdiv(int(pairs[l]), IVF_NQ) * _cdiv(int(offsets[l + 1] - offsets[l]), IVF_CHUNK) for l in range(nlist)))
    grid = 8 * torch.cuda.get_device_properties(DEV).multi_processor_count
    assert items == 40 * 75 * 2 and items > 2 * grid, (items, grid)
    assert Q > BASES_THREADS                                         # k_ivf_bases: a second workgroup
    x = _raw(10, Q, D)
    q, pt = _dev(x), _dev(p)
    S = _check_slab(ix, q, p, rows, x, offsets, order, f"{kind} D={D}")
    for k in (8, 150):
        v, i = ix.search(q, k, probes=pt)
        wv, wi, gap = I.topk(S, k)
        assert_topk_matches(_np(v), _np(i), wv, wi, gap=gap, what=f"{kind} D={D} k={k}", scores_ref=S)
        v7, i7 = ix.search(q, k, probes=pt, block=7)                 # 43 scans of at most 7 queries: no second item anywhere
        assert (_bits(v7) == _bits(v)).all() and (_bits(i7) == _bits(i)).all(), (kind, D, k)
    # one filtered case
    qlab = np.random.default_rng(4).integers(0, 4, Q)
    ex = _np(ix.search(q, 1, probes=pt)[1])[:, 0].copy()
    ex[::5] = -1
    Sf = I.restricted_scores(rows, x, offsets, order, p, query_labels=qlab, gallery_labels=glab, label_filter="different", exclude=ex)
    v, i = ix.search(q, 8, probes=pt, query_labels=_dev(qlab), label_filter="different", exclude=_dev(ex))
    v, i = _np(v), _np(i)
    wv, wi, gap = I.topk(Sf, 8)
    assert np.isfinite(np.take_along_axis(Sf, np.where(i >= 0, i, 0), axis=1))[i >= 0].all() and not (i == ex[:, None]).any()
    assert_topk_matches(v, i, wv, wi, gap=gap, what=f"{kind} D={D} filtered", scores_ref=Sf)


# ---- b. more lists than k_ivf_plan has threads
def _plan_lists(nlist):
    """The non-empty lists of an index of ``nlist`` lists, most of them empty: the first and the last list, the lists on
    either side of thread 1023 / 1024 of one-list runs, both sides of several boundaries between the runs of cdiv(nlist, 1024)
    lists that one thread of k_ivf_plan takes, and one whole run."""
    per = _cdiv(nlist, PLAN_THREADS)
    ids = {0, 1023, nlist - 1}
    if nlist > 1024:
        ids.add(1024)
    for t in (5, 170, 340, 832):                                     # the last list of run t and the first of run t + 1
        ids.update({per * t + per - 1, per * t + per})
    ids.update(range(per * 100, per * 100 + max(per, 3)))            # a whole run (at least three consecutive lists)
    return per, sorted(i for i in ids if i < nlist)


@pytest.mark.parametrize("nlist", [1024, 1025, 2500])
def test_ivf_plan_with_more_lists_than_threads(nlist):
    G, D, Q = 3000, 64, 9
    per, lists = _plan_lists(nlist)
    assert per == {1024: 1, 1025: 2, 2500: 3}[nlist] and {0, 1023, nlist - 1} <= set(lists) and (nlist == 1024 or 1024 in lists)
    if per == 3:
        assert all({3 * t + 2, 3 * t + 3} <= set(lists) for t in (5, 170, 340, 832)) and {300, 301, 302} <= set(lists)
    lengths = [1, 63, 64, 65, 3, 130] * len(lists)
    lengths = lengths[: len(lists)]
    lengths[-1] += G - sum(lengths)                                  # the last list takes the rest
    assert len(lists) < 20 and lengths[-1] > 64 and nlist - len(lists) > 1000       # most lists are empty
    assign = np.repeat(np.array(lists), lengths)[np.random.default_rng(7).permutation(G)].astype(np.int64)
    g = M.Gallery(D, DEV).add(_dev(_raw(1, G, D)))
    ix = M.IVFIndex(g, _dev(_raw(2, nlist, D)), _dev(assign))
    offsets, order = I.lists_of(assign, nlist)
    assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
    rows = _np(g.data.float()).astype(np.float64)
    x = _raw(10, Q, D)
    q = _dev(x)
    empties = np.setdiff1d(np.arange(nlist), lists)
    for nprobe in (1, 64, 1024):
        rng = np.random.default_rng(nprobe)
        p = np.empty((Q, nprobe), np.int64)
        for qi in range(Q):                                          # the non-empty lists rotated by the query, among empty ones
            mine = np.roll(lists, -qi)[:nprobe]
            row = np.concatenate([mine, rng.permutation(empties)[: nprobe - mine.size]])
            p[qi] = row[rng.permutation(nprobe)] if nprobe > 1 else row
        assert all(len(set(r)) == nprobe for r in p.tolist())
        S = _check_slab(ix, q, p, rows, x, offsets, order, f"nlist={nlist} nprobe={nprobe}")
        assert np.isfinite(S).any(axis=1).all()
        for k in (3, 150):
            v, i = ix.search(q, k, probes=_dev(p))
            wv, wi, gap = I.topk(S, k)
            assert_topk_matches(_np(v), _np(i), wv, wi, gap=gap, what=f"nlist={nlist} nprobe={nprobe} k={k}", scores_ref=S)


# ---- c. IVF-PQ and residual IVF-PQ: many probes, long runs of empty lists, the largest LDS
NLIST = 1100
LISTS = {7: 1, 300: 3, 555: 2047, 1023: 2048, 1099: 2049}           # the non-empty lists and their lengths: the chunk is 2048
G_PQ = sum(LISTS.values())
NPROBES = (63, 64, 65, 130, 257, 1024)
SHAPES = [(128, 128), (256, 128), (64, 8)]                           # (D, M): 1024 threads with dsub 1 and 2, 256 threads
KS = (1, 8, 9, 150)
NQ = 40


def _threads(Mq):
    return 256 if Mq <= 40 else 512 if Mq <= 80 else 1024            # of the scan's workgroup (pq_scan.h's dispatch)


@functools.lru_cache(maxsize=None)
def _pq_assign():
    a = np.empty(G_PQ, np.int64)
    a[np.random.RandomState(5).permutation(G_PQ)] = np.repeat(list(LISTS), list(LISTS.values()))
    return a


@functools.lru_cache(maxsize=None)
def _pq_probes(nprobe):
    """(NQ, nprobe): one order of nprobe distinct lists - the five non-empty ones min(205, nprobe // 5) apart, empty lists in
    between (at nprobe = 1024: runs of 204 empty lists, and 203 at the end) - rotated by 37 q for query q, so that the runs
    lead, trail and wrap."""
    gap = min(205, nprobe // 5)
    base = np.random.default_rng(nprobe).permutation(np.setdiff1d(np.arange(NLIST), list(LISTS)))[:nprobe].astype(np.int64)
    base[np.arange(5) * gap] = list(LISTS)
    assert len(set(base.tolist())) == nprobe
    if nprobe == 1024:
        runs = np.diff(np.concatenate([np.nonzero(np.isin(base, list(LISTS)))[0], [nprobe]])) - 1
        assert (runs >= 200).all()
    return np.stack([np.roll(base, -(37 * qi) % nprobe) for qi in range(NQ)])


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed)).to(DEV)


def _pq_parts(D, Mq):
    x, q = _randn((G_PQ, D), 100 + D + Mq), _randn((NQ, D), 200 + D + Mq)
    cb = (_randn((Mq, 256, D // Mq), 300 + D + Mq) / float(np.sqrt(D))).contiguous()
    cen = M.l2_normalize_rows(_randn((NLIST, D), 400 + D + Mq))
    lab = torch.randint(0, 4, (G_PQ,), generator=torch.Generator().manual_seed(D)).to(DEV)
    return x, q, cb, cen, lab


def _limits_search(ix, s, q, lab, D, Mq, what):
    """Every (nprobe, Q, k) of NPROBES x (1, NQ) x KS against the model's scores ``s`` (NQ, G_PQ), and one filtered case."""
    assign = _pq_assign()
    for nprobe in NPROBES:
        p = _pq_probes(nprobe)
        if nprobe > COARSE_CHUNK:
            assert _cdiv(nprobe, COARSE_CHUNK) >= 2                  # k_ivfpq_coarse: blockIdx.x >= 1 runs
        mask = V.probed_mask(assign, NLIST, p)
        wv, wi = R.topk(s, max(KS), mask)
        for Q in (1, NQ):
            for k in KS:
                v, i = ix.search(q[:Q], k, probes=_dev(p[:Q]))
                assert (_np(i) == wi[:Q, :k]).all(), f"{what} nprobe={nprobe} Q={Q} k={k}"
                _assert_bits(v, wv[:Q, :k], f"{what} nprobe={nprobe} Q={Q} k={k}")
    # the largest nprobe: the staging loops take a second trip (thread 0 at least), and at M = 128 the LDS is the declared maximum
    nprobe = max(NPROBES)
    assert nprobe == ivfpq_max_nprobe() and nprobe + 1 > _threads(Mq)
    p, off = _pq_probes(nprobe), 700
    ql = np.arange(NQ) % 4
    mask = V.probed_mask(assign, NLIST, p)
    ex = np.where(np.arange(NQ) % 3 == 1, -1, R.topk(s, 1, mask)[1][:, 0] + off)
    ok = I.eligible(G_PQ, NQ, ql, _np(lab), "different", ex, off)
    for k in (8, 9):
        wv, wi = R.topk(s, k, mask & ok)
        v, i = ix.search(q, k, probes=_dev(p), idx_offset=off, query_labels=_dev(ql), label_filter="different", exclude=_dev(ex))
        assert (_np(i) == np.where(wi >= 0, wi + off, -1)).all(), f"{what} filtered k={k}"
        _assert_bits(v, wv, f"{what} filtered k={k}")


def ivfpq_max_nprobe():
    return 1024                                                      # IVFPQ_MAX_NPROBE (ivfpq.hip), the bound of _lists.MAX_K


@pytest.mark.parametrize("D,Mq", SHAPES)
def test_ivfpq_many_probes_and_empty_runs(D, Mq):
    x, q, cb, cen, lab = _pq_parts(D, Mq)
    gal = pq.PQGallery(D, DEV, Mq, codebooks=cb).add(x, lab)
    ix = ivfpq.IVFPQIndex(gal, cen, _dev(_pq_assign()))
    offsets, order = I.lists_of(_pq_assign(), NLIST)
    assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
    s = R.scores(R.table(_np(M.l2_normalize_rows(q)), _np(cb)), _np(gal.codes))
    _limits_search(ix, s, q, lab, D, Mq, f"ivfpq D={D} M={Mq}")


@pytest.mark.parametrize("D,Mq", SHAPES)
def test_residual_ivfpq_many_probes_and_empty_runs(D, Mq):
    x, q, cb, cen, lab = _pq_parts(D, Mq)
    assign = _pq_assign()
    ix = ivfrpq.ResidualIVFPQIndex(cen, cb).add(x, lab, assignments=_dev(assign))
    offsets, order = I.lists_of(assign, NLIST)
    assert (_np(ix.offsets) == offsets).all() and (_np(ix.order) == order).all()
    # every (query, list) term from the rescoring routine over the centroids, all lists in order: the model's input
    L = _lib.lib()
    every = torch.arange(NLIST, dtype=torch.int64, device=DEV).repeat(NQ, 1).contiguous()
    coarse = torch.empty((NQ, NLIST), dtype=torch.float32, device=DEV)
    ws = torch.empty(L.mi355_rescore_candidates_workspace_bytes(NQ, D), dtype=torch.uint8, device=DEV)
    _lib.check(L.mi355_rescore_candidates(q.data_ptr(), NQ, D, ix.pq.eps, cen.data_ptr(), _lib.DTYPE_F32, D, NLIST,
                                          every.data_ptr(), NLIST, 0, coarse.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(torch.device(DEV))))
    coarse = _np(coarse)
    qn = _np(M.l2_normalize_rows(q))
    assert np.abs(coarse - qn.astype(np.float64) @ _np(cen).astype(np.float64).T).max() <= SCORE_TOL
    for nprobe in (65, 130, 1024):                                   # index.coarse over permuted probes: the same bits per pair
        p = _pq_probes(nprobe)
        _assert_bits(ix.coarse(q, _dev(p)), np.take_along_axis(coarse, p, axis=1), f"coarse nprobe={nprobe}")
    s = V.scores(coarse, qn, _np(cb), _np(ix.codes), assign)
    _limits_search(ix, s, q, lab, D, Mq, f"ivfrpq D={D} M={Mq}")
