"""Diffusion re-ranking on the GPU against the NumPy model (tests/diffusion_ref.py), stage by stage on the GPU's own inputs: the
graph stage (cols bit for bit, vals / deg to fp32 rounding, vals bit-symmetric), the solve (against float64 CG within a tolerance
sized by the model's own fp32 restatement), ``Gallery.diffuse`` end to end on fp32, fp16 and prepared galleries, bit-for-bit
properties, the edges, and the arcs R-precision gain through the public API."""
import functools

import numpy as np
import pytest
import torch

import diffusion_ref as dr
import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import diffusion as D
from imageretrievalresearch_amd import rerank as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = 37
ALPHA, GAMMA = 0.99, 3
# (L, kd, kq, iters): 257 gives the 256-thread row loops a second trip, 1024 and 32 are the limits
CASES = [(64, 8, 5, 20), (257, 32, 5, 20), (257, 32, 5, 64), (1024, 32, 10, 20), (1024, 16, 1024, 64), (480, 5, 1, 1), (64, 1, 5, 20)]
INDEX_CASES = CASES[:4]            # the last two are tie-heavy by construction: checked by value only
ULP = 2.0 ** -24


def _np(t):
    return t.cpu().numpy()


def _gallery(x, kind):
    x = torch.as_tensor(x).to(DEV)
    if kind == "fp16":
        return M.Gallery(x.shape[1], DEV, dtype=torch.float16).add(x)
    gal = M.Gallery(x.shape[1], DEV).add(x)
    return gal.prepare() if kind == "prepared" else gal


@functools.lru_cache(maxsize=None)
def _clustered():
    """300 x 70 rows of 20 clusters with a block of exactly duplicated rows (10 .. 17), as tests/test_rerank_gpu.py's _sets_case."""
    g = torch.Generator().manual_seed(11)
    centers = torch.randn(20, 70, generator=g)
    x = centers[torch.randint(0, 20, (300,), generator=g)] + torch.randn(300, 70, generator=g)
    x[10:18] = x[10]
    return x


@functools.lru_cache(maxsize=None)
def _arcs(narcs):
    rows, labels = dr.arcs(narcs)
    q, own, ql = dr.arc_queries(rows, narcs, 40, Q)
    return rows, labels, q, own, ql


@functools.lru_cache(maxsize=None)
def _arc_gallery(narcs, kind):
    return _gallery(_arcs(narcs)[0], kind)


# ---------------------------------------------------------------------------------------------- the graph stage
@pytest.mark.parametrize("gamma", [1, 3])
@pytest.mark.parametrize("kd", [1, 5, 32])
@pytest.mark.parametrize("rows", ["clustered", "arcs"])
def test_graph_stage(rows, kd, gamma):
    gal = _gallery(_clustered(), "fp32") if rows == "clustered" else _arc_gallery(12, "fp32")
    nv, nn = gal.knn_graph(kd)
    cols, vals, deg = (_np(t) for t in D._df_graph(nn, nv, gamma))
    wc, wv, wd = dr.graph(_np(nn), _np(nv), gamma)
    assert cols.dtype == np.int32 and np.array_equal(cols, wc), (rows, kd, gamma)
    assert (cols >= 0).any()
    # kd + 2 gamma + 5 fp32 roundings at most (<= 53 at the limits); below the normal range fp32 has no relative precision
    tiny = 2.0 ** -126
    ev = np.abs(vals - wv) - 64 * ULP * np.abs(wv)
    ed = np.abs(deg - wd) - 64 * ULP * np.abs(wd)
    print(f"{rows} kd={kd} gamma={gamma}: vals off by {np.max(np.abs(vals - wv) / np.maximum(np.abs(wv), tiny)) / ULP:.1f} ulp, "
          f"deg by {np.max(np.abs(deg - wd) / np.maximum(np.abs(wd), tiny)) / ULP:.1f} ulp; {(cols >= 0).mean():.2f} of the slots mutual")
    assert ev.max() <= tiny and ed.max() <= tiny
    assert (vals[cols < 0] == 0).all()
    S = dr.dense(cols, vals)
    assert S.dtype == np.float32 and np.array_equal(S.view(np.uint32), S.T.copy().view(np.uint32))     # i -> j and j -> i: the same bits


# ---------------------------------------------------------------------------------------------- the solve, and end to end
@functools.lru_cache(maxsize=None)
def _run(kind, case):
    """One gallery kind and one (L, kd, kq, iters): what the GPU gives at every stage, and the model fed the GPU's own index rows,
    shortlist and source vector.  Computed once, shared by the tests below, never changed."""
    L, kd, kq, iters = case
    narcs = 30 if L > 480 else 12
    _, _, q, own, _ = _arcs(narcs)
    gal = _arc_gallery(narcs, kind)
    qd, ex = torch.from_numpy(q).to(DEV), torch.from_numpy(own).to(DEV)
    index = gal.diffusion_index(kd, GAMMA)
    sv, si = K._shortlist_search(gal, qd, L, ex)
    sv, si = sv.contiguous(), si.contiguous()
    y = D._df_source(sv, si, kq, GAMMA)
    f, its = D._df_solve(index.cols, index.vals, si, y, ALPHA, iters)
    cols, vals, si_np, y_np = _np(index.cols), _np(index.vals), _np(si), _np(y)
    f64, its64 = dr.solve(cols, vals, si_np, y_np, ALPHA, iters)
    f32, _ = dr.solve(cols, vals, si_np, y_np, ALPHA, iters, np.float32)
    scale = np.abs(np.where(np.isfinite(f64), f64, 0)).max(axis=1)
    with np.errstate(invalid="ignore"):
        e32 = np.nanmax(np.where(np.isfinite(f64), np.abs(f32 - f64), 0).max(axis=1) / scale)
    out = gal.diffuse(qd, 10, kd=kd, kq=kq, alpha=ALPHA, gamma=GAMMA, iters=iters, shortlist=L, exclude=ex, stats=True)
    return dict(f=_np(f), its=_np(its), f64=f64, its64=its64, e32=float(e32), tol=max(8 * float(e32), 1e-5), scale=scale, sv=_np(sv),
                si=si_np, y=y_np, out=tuple(_np(t) for t in out))


def _err(got, want, scale):
    """max |got - want| / scale per query over the finite entries; the -inf of the pads must coincide."""
    pad = ~np.isfinite(want)
    assert np.array_equal(np.isneginf(got), pad)
    return np.where(pad, 0, np.abs(np.where(pad, 0, got) - np.where(pad, 0, want))).max(axis=1) / scale


@pytest.mark.parametrize("case", CASES, ids=str)
def test_solve_stage(case):
    L, kd, kq, iters = case
    r = _run("fp32", case)
    wy = dr.source(r["sv"], r["si"], kq, GAMMA)
    assert (np.abs(r["y"] - wy) <= (GAMMA + 1) * ULP * np.abs(wy)).all() and (r["y"][:, kq:] == 0).all()
    err = _err(r["f"], r["f64"], r["scale"])
    print(f"L={L} kd={kd} kq={kq} iters={iters}: e32 {r['e32']:.2e}, TOL {r['tol']:.2e}, GPU error {err.max():.2e}; iterations "
          f"GPU {r['its'].min()}..{r['its'].max()}, float64 {r['its64'].min()}..{r['its64'].max()}")
    assert err.max() <= r["tol"]
    assert (r["its"] >= 1).all() and (r["its"] <= iters).all()
    if L == 480:                                                   # every row of the gallery but the query's own: one pad, last
        assert (r["si"][:, -1] == -1).all() and np.isneginf(r["f"][:, -1]).all() and (r["its"] == 1).all()


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("kind", ["fp32", "fp16", "prepared"])
def test_end_to_end(kind, case):
    r = _run(kind, case)
    vals, idx, its = r["out"]
    wv, wi, _ = dr.rank_shortlist(r["f64"], r["si"], 10)
    assert vals.shape == (Q, 10) and idx.shape == (Q, 10) and np.array_equal(its, r["its"])
    err = np.abs(vals - wv).max(axis=1) / r["scale"]
    assert err.max() <= r["tol"], (kind, case, err.max(), r["tol"])
    # every returned row is a shortlist row and carries its own f
    pos = np.array([[list(r["si"][q]).index(i) for i in idx[q]] for q in range(Q)])
    assert np.array_equal(np.take_along_axis(r["f"], pos, 1), vals)
    if case in INDEX_CASES:
        sure = ~dr.close_pairs(r["f64"], 10)
        print(f"{kind} {case}: {int((~sure).sum())} of {sure.size} positions next to a near-tie are not compared")
        assert (~sure).mean() <= 0.05
        assert np.array_equal(idx[sure], wi[sure]), (kind, case)


# ---------------------------------------------------------------------------------------------- properties, bit for bit
def _prop():
    _, _, q, own, _ = _arcs(12)
    return _arc_gallery(12, "fp32"), torch.from_numpy(q).to(DEV), torch.from_numpy(own).to(DEV)


KW = dict(kd=8, kq=5, shortlist=100, stats=True)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def test_the_same_call_twice_and_every_batch_size():
    gal, q, own = _prop()
    full = gal.diffuse(q, 10, exclude=own, **KW)
    assert _same(full, gal.diffuse(q, 10, exclude=own, **KW))
    for n in (1, 4, 5):
        part = gal.diffuse(q[:n], 10, exclude=own[:n], **KW)
        assert _same(part, tuple(t[:n] for t in full)), n
    alone = gal.diffuse(q[20:21], 10, exclude=own[20:21], **KW)
    assert _same(alone, tuple(t[20:21] for t in full))


def test_gallery_diffuse_equals_diffusion_rerank():
    gal, q, own = _prop()
    rows = torch.from_numpy(_arcs(12)[0]).to(DEV)
    assert _same(gal.diffuse(q, 10, exclude=own, **KW), M.diffusion_rerank(q, rows, 10, exclude=own, **KW))
    assert _same(gal.diffuse(q, 7), D.diffusion_rerank(q, rows, 7))


def test_the_index_is_cached_and_dropped_by_add():
    rows = torch.from_numpy(_arcs(12)[0]).to(DEV)
    gal = M.Gallery(32, DEV).add(rows[:400])
    ix = gal.diffusion_index(8, 3)
    assert gal.diffusion_index(8, 3) is ix and gal.diffusion_index(8, 2) is not ix and gal.diffusion_index(9) is not ix
    assert isinstance(ix, M.DiffusionIndex) and (ix.kd, ix.gamma, ix.rows) == (8, 3, 400)
    assert ix.nbytes == 400 * 8 * (8 + 4 + 4 + 4) + 400 * 4
    assert ix.nn is gal.knn_graph(8)[1]                            # the gallery's cached graph, not a second one
    gal.add(rows[400:])
    assert gal.diffusion_index(8, 3) is not ix and gal.diffusion_index(8, 3).rows == 480


# ---------------------------------------------------------------------------------------------- edges
def test_full_shortlist_with_exclude_ends_in_one_pad():
    gal, q, own = _prop()
    v, i = gal.diffuse(q, 480, kd=8, shortlist=480, exclude=own)
    v, i = _np(v), _np(i)
    assert np.isneginf(v[:, -1]).all() and (i[:, -1] == -1).all() and np.isfinite(v[:, :-1]).all()
    for qi in range(Q):
        assert sorted(i[qi, :-1]) == [r for r in range(480) if r != _np(own)[qi]]
    assert (np.diff(v, axis=1) <= 0).all()


def test_a_query_with_no_positive_score_keeps_the_shortlist_order():
    g = torch.Generator().manual_seed(3)
    rows = torch.rand(100, 16, generator=g).to(DEV) + 0.1           # every coordinate positive
    gal = M.Gallery(16, DEV).add(rows)
    q = torch.cat([-torch.ones(1, 16), torch.ones(1, 16)]).to(DEV)
    v, i, its = gal.diffuse(q, 10, kd=5, shortlist=50, stats=True)
    sv, si = gal.search(torch.cat([q, q[-1:].expand(3, -1)]), 50)  # the shortlist search of the call above
    assert bool((sv[0] <= 0).all())
    assert its.tolist()[0] == 0 and its.tolist()[1] >= 1
    assert torch.equal(i[0], si[0, :10]) and bool((v[0] == 0).all())   # y = 0: f = 0, ties to the earlier position
    assert bool((v[1] > 0).all())


def test_rows_without_a_mutual_edge_keep_their_source_value():
    r = _run("fp32", (64, 1, 5, 20))
    gal = _arc_gallery(12, "fp32")
    cols = _np(gal.diffusion_index(1, GAMMA).cols)
    alone = (cols[np.maximum(r["si"], 0)] < 0).all(axis=2) & (r["si"] >= 0)      # (Q, L): no edge at all
    assert alone.any() and not alone.all() and alone[:, :5].any()
    # an isolated row is its own 1 x 1 system, f = y; the error is measured as everywhere else in this file
    err = np.abs(np.where(alone, r["f"] - r["y"], 0)).max(axis=1) / r["scale"]
    assert err.max() <= r["tol"]


def test_idx_offset_and_no_queries():
    gal, q, own = _prop()
    v0, i0 = gal.diffuse(q, 480, kd=8, shortlist=480, exclude=own)
    v1, i1 = gal.diffuse(q, 480, kd=8, shortlist=480, exclude=own + 1000, idx_offset=1000)
    assert torch.equal(v0, v1) and torch.equal(torch.where(i0 >= 0, i0 + 1000, i0), i1) and bool((i1[:, -1] == -1).all())
    out = gal.diffuse(q[:0], 6, stats=True)
    assert [tuple(t.shape) for t in out] == [(0, 6), (0, 6), (0,)]
    assert [t.dtype for t in out] == [torch.float32, torch.int64, torch.int32]
    assert [tuple(t.shape) for t in M.diffusion_rerank(q[:0], gal.data, 6)] == [(0, 6), (0, 6)]


def test_python_guards_on_device_tensors():
    gal, q, own = _prop()
    for kw in (dict(kd=33), dict(kq=0), dict(kq=201), dict(alpha=1.0), dict(alpha=float("nan")), dict(gamma=9), dict(iters=65),
               dict(shortlist=1025), dict(shortlist=5), dict(exclude=own[:3])):
        with pytest.raises(M.MI355Error):
            gal.diffuse(q, 10, **kw)
    with pytest.raises(M.MI355Error):
        gal.diffuse(q[:, :31], 10)
    i64 = torch.zeros(4, 3, dtype=torch.int64, device=DEV)
    with pytest.raises(M.MI355Error):
        D._df_solve(i64.int(), i64.float(), i64, torch.zeros(4, 2, device=DEV))      # y of another shape


# ---------------------------------------------------------------------------------------------- usefulness
def test_diffusion_follows_the_arcs():
    rows, labels, q, own, ql = _arcs(12)
    gal, qd, ex = _prop()
    plain = _np(gal.search(qd, 200, exclude=ex)[1])
    ranked = _np(gal.diffuse(qd, 200, kd=10, kq=5, shortlist=200, exclude=ex)[1])
    before, after = dr.r_precision(plain, labels, ql, own), dr.r_precision(ranked, labels, ql, own)
    print(f"arcs R-precision on the GPU: plain {before:.3f}, diffusion {after:.3f}")
    assert after >= before + 0.05
