"""Rows longer than one trip of the row walkers, on the GPU against float64 (int8: against the NumPy model, bit for bit).  The
shapes sit on the constants of the code (tests/long_rows_cases.py restates them): the second trip of row_dot (row_dot.h: the
IVF scan, mi355_rescore_candidates, the graph walk) and of the three GEMVs, every group size of ivf_group() and ivf_group_i8() with both sides of
each step, and both sides of each GEMV's LDS rule - the side past it being "Q <= 4, but the GEMM runs".  Each case asserts the
condition it is there for: the reported rank path, or the group size its dim implies.  test_long_rows_args.py shows without a
GPU that the reference keeps nine tenths of SCORE_TOL for the kernels and that a dropped, repeated or misplaced trip cannot
pass."""
import functools

import numpy as np
import pytest
import torch

import gallery_i8_ref as R8
import imageretrievalresearch_amd as M
import ivf_i8_ref as R8I
import ivf_ref as ref
import long_rows_cases as C
from helpers import SCORE_TOL, assert_topk_matches
from imageretrievalresearch_amd import _lib, ivf_i8
from imageretrievalresearch_amd import rank as _rank
from test_gallery_f16_gpu import _check_topk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16}
GEMV, SPLIT, F16_GEMM, F16_GEMV, I8_GEMM, I8_GEMV = 1, 2, 5, 6, 7, 8


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gallery(kind, D, G):
    """(gallery, its rows as stored in float64)."""
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(_dev(C.raw(kind, 1, G, D)))
    return g, g.data.float().cpu().numpy().astype(np.float64)


def _rescore_all(g, x):
    """(Q, rows) float32: mi355_rescore_candidates of every (query, row) pair."""
    Q, n, L = x.shape[0], g.rows, _lib.lib()
    cand = torch.arange(n, dtype=torch.int64, device=DEV).repeat(Q, 1).contiguous()
    out = torch.empty((Q, n), dtype=torch.float32, device=DEV)
    ws = torch.empty(max(1, L.mi355_rescore_candidates_workspace_bytes(Q, g.dim)), dtype=torch.uint8, device=DEV)
    _lib.check(L.mi355_rescore_candidates(x.data_ptr(), Q, g.dim, g.eps, g._buf.data_ptr(), _rank._DTYPES[g.dtype], g._ld, n,
                                          cand.data_ptr(), n, 0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(torch.device(DEV))))
    return out.cpu().numpy()


# ---- a. the anchor: row_dot through mi355_rescore_candidates (the graph tests take their score matrix from this entry)
@pytest.mark.parametrize("kind,D", [(k, D) for k in C.RESCORE_DIMS for D in C.RESCORE_DIMS[k]])
def test_rescore_candidates_past_the_first_trip(kind, D):
    first, unit = C.FIRST_TRIP[kind], C.UNIT[kind]
    trips = -(-(C.ldq(D, kind) // unit) // 256)                      # of the walk's 4 x 64 units
    assert trips == 1 if D == first else trips >= 2                  # the longest row of one trip, or a second trip
    g, rows = _gallery(kind, D, C.RESCORE_G)
    x = C.raw(kind, 2, C.RESCORE_Q, D)
    got = _rescore_all(g, _dev(x))
    want = ref.normalise(x) @ rows.T
    worst = float(np.abs(got - want).max())
    print(f"[long rows] rescore {kind} D={D}: max |score - f64| {worst:.3e}")
    assert worst <= SCORE_TOL


@pytest.mark.parametrize("kind", list(DTYPES))
def test_rescore_candidates_refuses_a_query_past_the_lds(kind):
    D = C.TOO_LONG
    assert C.ldq(D, kind) * 4 > 64 * 1024
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(_dev(C.raw(kind, 1, 8, D)))
    with pytest.raises(M.MI355Error, match="too large"):
        _rescore_all(g, _dev(C.raw(kind, 2, 2, D)))


# ---- b. the IVF scan at every group size
@functools.lru_cache(maxsize=None)
def _lists():
    a = C.ivf_assign()
    return (a,) + ref.lists_of(a, len(C.IVF_LENGTHS))


def _ivf(kind, D):
    a, offsets, order = _lists()
    g, rows = _gallery(kind, D, C.IVF_G)
    ix = M.IVFIndex(g, _dev(C.raw(kind, 3, len(C.IVF_LENGTHS), D)), _dev(a))
    assert (ix.offsets.cpu().numpy() == offsets).all() and (ix.order.cpu().numpy() == order).all()
    return ix, rows, offsets, order


@pytest.mark.parametrize("kind,D", [(k, D) for k in C.IVF_DIMS for D in C.IVF_DIMS[k]])
def test_ivf_scan_at_every_group_size(kind, D):
    nq = C.ivf_nq(D, kind)
    assert nq == C.IVF_NQ[D] and [len(g) for g in C.ivf_groups(nq)] == {4: [4, 4, 1], 3: [3, 3, 3], 2: [2, 2, 2, 2, 1], 1: [1] * 9}[nq]
    ix, rows, offsets, order = _ivf(kind, D)
    Q = C.IVF_Q
    x = C.raw(kind, 2, Q, D)
    q = _dev(x)
    p = np.tile(np.array(C.IVF_PROBES, np.int64), (Q, 1))            # the same lists for all: the groups are whole
    pt = _dev(p)
    S = ref.restricted_scores(rows, x, offsets, order, p)
    cap = int(ix._longest[p.shape[1]])
    cv, ci = (t.cpu().numpy() for t in ix._scan(q, pt, cap, 0, None))
    want = ref.probed_rows(offsets, order, p[0])
    assert want.size == C.IVF_G == cap
    worst = 0.0
    for i in range(Q):
        assert (ci[i] == want).all(), (kind, D, i)
        worst = max(worst, float(np.abs(cv[i] - S[i, want]).max()))
    print(f"[long rows] ivf {kind} D={D} nq={nq}: max |slab score - f64| {worst:.3e}")
    assert worst <= SCORE_TOL
    for k in (3, 9):
        v, i = ix.search(q, k, probes=pt)
        wv, wi, gap = ref.topk(S, k)
        assert_topk_matches(v.cpu().numpy(), i.cpu().numpy(), wv, wi, gap=gap, what=f"{kind} D={D} k={k}", scores_ref=S)
        # a query searched alone (a group of one) gives the bits it gives inside its group
        for j in range(Q):
            v1, i1 = ix.search(q[j: j + 1], k, probes=pt[j: j + 1])
            assert (_bits(v1[0]) == _bits(v[j])).all() and (_bits(i1[0]) == _bits(i[j])).all(), (kind, D, k, j)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_ivf_scan_refuses_a_query_past_the_lds(kind):
    D = C.TOO_LONG
    assert C.ivf_nq(D, kind) == 0 and C.ivf_nq(16384, kind) == 1
    a = np.arange(8, dtype=np.int64) % 2
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(_dev(C.raw(kind, 1, 8, D)))
    ix = M.IVFIndex(g, _dev(C.raw(kind, 3, 2, D)), _dev(a))
    with pytest.raises(M.MI355Error, match="too large"):
        ix.search(_dev(C.raw(kind, 2, 2, D)), 3, probes=_dev(np.array([[0, 1], [1, 0]], np.int64)))


@pytest.mark.parametrize("D", C.IVF_DIMS_I8)
def test_ivf_i8_scan_at_every_group_size(D):
    """Int8IVFIndex over the same five lists at every step of ivf_group_i8: the candidate slab and the search against the
    NumPy model of the int8 score restricted to the probed lists, bit for bit.  D = 32768: one query's planes are the whole
    64 KB of LDS."""
    nq, lq, Q = C.ivf_nq_i8(D), C.lq_i8(D), C.IVF_Q
    assert nq == C.IVF_GROUP_I8[D] and [len(g) for g in C.ivf_groups(nq)] == C.IVF_SPLIT_I8[nq]
    assert nq * 2 * lq <= C.IVF_LDS and (nq == C.IVF_MAXQ_I8 or (nq + 1) * 2 * lq > C.IVF_LDS)
    assert D != 32768 or (nq, 2 * lq) == (1, C.IVF_LDS)
    a, offsets, order = _lists()
    xt, q = _dev(C.raw("i8", 1, C.IVF_G, D)), _dev(C.raw("i8", 2, Q, D))
    gal = M.Int8Gallery(D, DEV).add(xt)
    assert gal._codes.shape[1] == lq
    ix = ivf_i8.Int8IVFIndex(gal, _dev(C.raw("i8", 3, len(C.IVF_LENGTHS), D)), _dev(a))
    assert (ix.offsets.cpu().numpy() == offsets).all() and (ix.order.cpu().numpy() == order).all()
    codes, s_g = R8.quantize_rows(M.l2_normalize_rows(xt).cpu().numpy())
    assert (gal.codes.cpu().numpy() == codes).all() and (_bits(gal.scales) == s_g.view(np.int32)).all()
    s = R8I.pair_scores(M.l2_normalize_rows(q).cpu().numpy(), codes, s_g)
    assert np.isfinite(s).all()
    p = np.tile(np.array(C.IVF_PROBES, np.int64), (Q, 1))            # the same lists for all: the groups are whole
    pt = _dev(p)
    want = ref.probed_rows(offsets, order, p[0])
    assert want.size == C.IVF_G and sorted(want.tolist()) == list(range(C.IVF_G))
    for cap in (C.IVF_G, C.IVF_G + 5):                               # the slab ends with the lists; five pads behind them
        cv, ci = ix._scan(q, pt, cap, 0, None)
        wv, wi = R8I.slab(s, offsets, order, p, cap)
        assert (wi[:, :C.IVF_G] == want[None, :]).all() and (wi[:, C.IVF_G:] == R8I.NO_CAND).all()
        assert (ci.cpu().numpy() == wi).all(), (D, cap)
        assert (_bits(cv) == wv.view(np.int32)).all(), (D, cap)
    for k in (3, 9):
        v, i = ix.search(q, k, probes=pt)
        wv, wi = R8I.search(s, offsets, order, p, k)
        assert (i.cpu().numpy() == wi).all() and (_bits(v) == wv.view(np.int32)).all(), (D, k)
        ev, ei = gal.search(q, k)                                    # every list probed: the exhaustive search's bits
        assert _path() == I8_GEMM, (D, k, _path())
        assert (_bits(ev) == _bits(v)).all() and (_bits(ei) == _bits(i)).all(), (D, k)
        # a query searched alone (a group of one) gives the bits it gives inside its group
        for j in range(Q):
            v1, i1 = ix.search(q[j: j + 1], k, probes=pt[j: j + 1])
            assert (_bits(v1[0]) == _bits(v[j])).all() and (_bits(i1[0]) == _bits(i[j])).all(), (D, k, j)


# ---- c. the three GEMVs, and the GEMM just past their LDS rules
def _path():
    return _lib.lib().mi355_rank_last_path() & 0xff


def _float_gemv_cases(kind, D, cases, gemv_path, gemm_path):
    g, rows = _gallery(kind, D, C.GEMV_G)
    if kind == "f16":
        assert g._ld == D
    x = C.raw(kind, 2, 64, D)
    q = _dev(x)
    S = torch.from_numpy(ref.normalise(x) @ rows.T)
    worst = 0.0
    for Q, gemv in cases:
        assert Q <= 4
        for k in (3, 9):
            v, i = g.search(q[:Q], k)
            assert _path() == (gemv_path if gemv else gemm_path), (kind, D, Q, k, _path())
            _check_topk(v, i, S[:Q], k, f"{kind} D={D} Q={Q} k={k}")
            worst = max(worst, float((v.cpu().double() - torch.gather(S[:Q], 1, i.cpu())).abs().max()))
            if not gemv:                                             # few queries on the GEMM: the same query alone, and among 64
                v1, i1 = g.search(q[:1], k)
                assert _path() == gemv_path, (kind, D, k)
                v64, i64 = g.search(q, k)
                assert _path() == gemm_path, (kind, D, k)
                _check_topk(v64, i64, S, k, f"{kind} D={D} Q=64 k={k}")
                for other in (v1[0], v64[0]):
                    assert float((other - v[0]).abs().max()) <= SCORE_TOL, (kind, D, k)
    print(f"[long rows] gemv {kind} D={D}: max |score - f64| {worst:.3e}")
    assert worst <= SCORE_TOL


@pytest.mark.parametrize("D", sorted({D for D, _ in C.GEMV_F16}))
def test_gemv_f16_past_the_first_trip_and_its_lds_rule(D):
    cases = [(Q, C.GEMV_F16[(D, Q)]) for Q in (1, 2, 3, 4)]
    assert [gemv for _, gemv in cases] == ([True, True, True, False] if D == 4160 else [True] * 4)
    _float_gemv_cases("f16", D, cases, F16_GEMV, F16_GEMM)


@pytest.mark.parametrize("D", sorted({D for D, _ in C.GEMV_F32}))
def test_gemv_f32_at_its_lds_rule(D):
    cases = [(Q, gemv) for (d, Q), gemv in C.GEMV_F32.items() if d == D]
    assert cases == {3840: [(4, True)], 3844: [(4, False)], 15360: [(1, True)]}[D]
    _float_gemv_cases("f32", D, cases, GEMV, SPLIT)


@pytest.mark.parametrize("D", sorted({D for D, _ in C.GEMV_I8}))
def test_gemv_i8_past_the_first_trip_and_its_lds_rule(D):
    x, qx = C.raw("i8", 1, C.GEMV_G, D), C.raw("i8", 2, 64, D)
    xt, q = _dev(x), _dev(qx)
    gal = M.Int8Gallery(D, DEV).add(xt)
    assert gal._codes.shape[1] == D
    codes, s_g = R8.quantize_rows(M.l2_normalize_rows(xt).cpu().numpy())
    assert (gal.codes.cpu().numpy() == codes).all()
    hi, lo, s_q = R8.query_planes(M.l2_normalize_rows(q).cpu().numpy())
    wv, wi = R8.topk(R8.scores(hi, lo, s_q, codes, s_g), 9)
    assert (C.GEMV_I8[(D, 1)], C.GEMV_I8[(D, 4)]) == (True, D <= 8192)
    for Q in (1, 4):
        gemv = C.GEMV_I8[(D, Q)]
        for k in (3, 9):
            v, i = gal.search(q[:Q], k)
            assert _path() == (I8_GEMV if gemv else I8_GEMM), (D, Q, k, _path())
            assert (_bits(v) == wv[:Q, :k].view(np.int32)).all() and (i.cpu().numpy() == wi[:Q, :k]).all(), (D, Q, k)
            if not gemv:                                             # the GEMM among 64 queries: the same bits again
                v64, i64 = gal.search(q, k)
                assert _path() == I8_GEMM
                assert (_bits(v64) == wv[:, :k].view(np.int32)).all() and (i64.cpu().numpy() == wi[:, :k]).all(), (D, k)
