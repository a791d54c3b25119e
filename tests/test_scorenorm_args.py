"""Score normalisation without a GPU: the new symbols are declared, bound and exported; every argument check of the adjusted
entries and of mi355_topn_stats (rejected before any HIP call, with a message); the checks of the Python API; and where the
public names live.  No device is touched: the pointers handed to the C entries are never dereferenced."""
import ctypes as C
import math

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib
from imageretrievalresearch_amd import rank as R
from imageretrievalresearch_amd import scorenorm as S

NAMES = ["mi355_rank_adjusted_workspace_bytes", "mi355_rank_adjusted_f16_workspace_bytes", "mi355_rank_topk_adjusted",
         "mi355_rank_topk_adjusted_f16", "mi355_cosine_scores_adjusted", "mi355_cosine_scores_adjusted_f16", "mi355_topn_stats"]
BIG = 1 << 40            # a workspace size no check finds short


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_are_declared_bound_and_exported():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert _lib.lib().mi355_abi_version() == 3


def _adjust(aq=16, bq=16, ag=16, bg=16):
    a = _lib.ScoreAdjust()
    a.aq, a.bq, a.ag, a.bg = aq, bq, ag, bg
    return a


def _topk(f16=False, q=16, Q=8, g=16, G=300, dim=48, k=3, adjust="default", filt=None, qblock=0, val=16, idx=16, ws=16, ws_bytes=BIG):
    L = _lib.lib()
    a = _adjust() if adjust == "default" else adjust
    ap = None if a is None else C.byref(a)
    fp = None if filt is None else C.byref(filt)
    if f16:
        return L.mi355_rank_topk_adjusted_f16(q, Q, g, G, dim, k, 1e-6, 0, ap, fp, qblock, val, idx, ws, ws_bytes, None)
    return L.mi355_rank_topk_adjusted(q, Q, g, G, dim, 1, k, 1e-6, 0, ap, fp, qblock, val, idx, ws, ws_bytes, None)


def _scores(f16=False, q=16, Q=8, g=16, G=300, dim=48, adjust="default", qblock=0, out=16, ws=16, ws_bytes=BIG):
    L = _lib.lib()
    a = _adjust() if adjust == "default" else adjust
    ap = None if a is None else C.byref(a)
    if f16:
        return L.mi355_cosine_scores_adjusted_f16(q, Q, g, G, dim, 1e-6, ap, qblock, out, ws, ws_bytes, None)
    return L.mi355_cosine_scores_adjusted(q, Q, g, G, dim, 1, 1e-6, ap, qblock, out, ws, ws_bytes, None)


def _bad_filter():
    f = _lib.RankFilter()
    f.label_mode = _lib.LABEL_SAME            # without labels
    return f


TOPK_CASES = [
    (dict(q=None), b"null"), (dict(g=None), b"null"), (dict(adjust=None), b"null adjust"), (dict(val=None), b"null output"),
    (dict(idx=None), b"null output"), (dict(adjust=_adjust(aq=None, ag=None)), b"aq and ag are both null"),
    (dict(k=0), b"k=0 outside [1,1024]"), (dict(k=1025, G=2000), b"k=1025 outside [1,1024]"), (dict(k=301), b"k=301 exceeds gallery rows 300"),
    (dict(ws_bytes=64), b"workspace 64 <"), (dict(ws=None), b"workspace"), (dict(Q=-1), b"Q=-1"), (dict(G=0), b"G=0"),
    (dict(dim=0), b"dim=0"), (dict(qblock=-1), b"query_block=-1"), (dict(filt=_bad_filter()), b"needs query_labels"),
]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("kw, msg", TOPK_CASES)
def test_topk_entries_reject_bad_arguments(f16, kw, msg):
    assert _topk(f16, **kw) != 0
    assert msg in _err(), (kw, _err())


def test_fp16_rows_must_be_16_byte_aligned():
    assert _topk(True, g=8) != 0 and b"16-byte aligned" in _err()
    assert _scores(True, g=24) != 0 and b"16-byte aligned" in _err()
    assert _topk(False, g=8, ws_bytes=64) != 0 and b"workspace" in _err()      # fp32 rows: no such rule, the next check speaks


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("kw, msg", [
    (dict(q=None), b"null"), (dict(g=None), b"null"), (dict(adjust=None), b"null adjust"), (dict(out=None), b"null output"),
    (dict(adjust=_adjust(aq=None, ag=None)), b"aq and ag are both null"), (dict(ws_bytes=64), b"workspace 64 <"),
    (dict(ws=None), b"workspace"), (dict(G=0), b"G=0"), (dict(dim=0), b"dim=0"), (dict(qblock=-1), b"query_block=-1"),
])
def test_slab_entries_reject_bad_arguments(f16, kw, msg):
    assert _scores(f16, **kw) != 0
    assert msg in _err(), (kw, _err())


def test_one_vector_of_each_pair_is_enough_and_zero_queries_do_nothing():
    # (the argument checks pass and the workspace check is the one that speaks: nothing is launched)
    for a in (_adjust(aq=None, bq=None), _adjust(ag=None, bg=None), _adjust(bq=None, bg=None)):
        assert _topk(adjust=a, ws_bytes=64) != 0 and b"workspace" in _err()
    assert _topk(Q=0) == 0 and _topk(True, Q=0) == 0 and _scores(Q=0) == 0 and _scores(True, Q=0) == 0


def test_the_workspace_sizers():
    L = _lib.lib()
    # the fused selection keeps no Q x G slab, adjusted or not; k > 8 and Q <= 4 select from the adjusted slab
    assert L.mi355_rank_adjusted_workspace_bytes(256, 100000, 1536, 3) == L.mi355_rank_workspace_bytes(256, 100000, 1536, 3)
    assert L.mi355_rank_adjusted_workspace_bytes(256, 100000, 1536, 3) < 16 * 2**20
    assert L.mi355_rank_adjusted_workspace_bytes(256, 100000, 1536, 150) > 256 * 100000 * 4
    assert L.mi355_rank_adjusted_workspace_bytes(4, 100000, 1536, 3) > 4 * 100000 * 4
    assert L.mi355_rank_adjusted_f16_workspace_bytes(256, 100000, 1536, 3) < 16 * 2**20
    # no GEMV: one query carries its planes
    assert L.mi355_rank_adjusted_f16_workspace_bytes(1, 100000, 1536, 3) > L.mi355_rank_f16_workspace_bytes(1, 100000, 1536, 3)
    for fn in (L.mi355_rank_adjusted_workspace_bytes, L.mi355_rank_adjusted_f16_workspace_bytes):
        assert fn(5, 300, 48, 0) > 0
        assert fn(0, 300, 48, 3) == 0 and fn(5, 0, 48, 3) == 0 and fn(5, 300, 0, 3) == 0 and fn(5, 300, 48, -1) == 0
        assert fn(5, 300, 48, 1025) == 0


def _stats(val=16, idx=16, N=4, n=10, half=1.0, min_std=1e-6, mean=16, std=16, count=16, a=None, b=None):
    return _lib.lib().mi355_topn_stats(val, idx, N, n, half, min_std, mean, std, count, a, b, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(val=None), b"null"), (dict(idx=None), b"null"), (dict(mean=None), b"null"), (dict(std=None), b"null"),
    (dict(count=None), b"null"), (dict(a=16), b"a and b go together"), (dict(b=16), b"a and b go together"), (dict(N=-1), b"N=-1"),
    (dict(N=1 << 31), b"N="), (dict(n=0), b"n=0"), (dict(n=1025), b"n=1025"), (dict(half=math.nan), b"half"),
    (dict(half=math.inf), b"half"), (dict(min_std=-1.0), b"min_std"), (dict(min_std=math.nan), b"min_std"),
])
def test_stats_entry_rejects_bad_arguments(kw, msg):
    assert _stats(**kw) != 0
    assert msg in _err(), (kw, _err())


def test_stats_of_no_rows_do_nothing():
    assert _stats(N=0) == 0 and _stats(N=0, a=16, b=16, n=1024, half=0.5, min_std=0.0) == 0


# ---------------------------------------------------------------------------------------------- the Python API
def _norm(kind="znorm", rows=5, **kw):
    one = torch.ones(rows)
    coef = {"csls": dict(bg=one), "znorm": dict(ag=one, bg=one), "tnorm": {}, "snorm": dict(ag=one, bg=one)}[kind]
    cohort = R._Rows(torch.zeros(7, 8), 7, 8, True) if kind in ("tnorm", "snorm") else None
    return S.ScoreNorm(kind, rows, **{**coef, "cohort": cohort, **kw})


def test_an_unknown_kind():
    for kind in ("cosine", "CSLS", None, 3):
        with pytest.raises(MI355Error, match="kind must be one of"):
            S.ScoreNorm(kind, 5, bg=torch.ones(5))
        with pytest.raises(MI355Error, match="kind must be one of"):
            S.ScoreNorm.fit(R.Gallery(8, "cpu"), torch.zeros(3, 8), kind)
        with pytest.raises(MI355Error, match="kind must be one of"):
            R.Gallery(8, "cpu").score_norm(torch.zeros(3, 8), kind)
    for kind in S.KINDS:
        assert _norm(kind).kind == kind


def test_n_out_of_range():
    assert _norm("csls", rows=50).n == 10 and _norm("csls", rows=5).n == 5          # CSLS: 10, capped at the rows
    assert _norm("snorm").n == 7 and _norm("tnorm", n=3).n == 3                   # the norms: the whole cohort, or the top n
    for kind, n in (("csls", 0), ("csls", 6), ("csls", 2.0), ("csls", True), ("snorm", 8), ("tnorm", 0), ("tnorm", -1), ("znorm", 1025)):
        with pytest.raises(MI355Error, match="n must be an integer in"):
            _norm(kind, n=n)
    with pytest.raises(MI355Error, match="n must be an integer in"):                # None is the whole cohort: at most 1024 rows
        S._cohort_n(None, 5000)
    assert S._cohort_n(None, 5000, 10) == 10 and S._cohort_n(1024, 5000) == 1024 and S._cohort_n(None, 300) == 300
    for n in (0, 301, 1025, 1.5, "3", False):
        with pytest.raises(MI355Error, match="n must be an integer in"):
            S._cohort_n(n, 300)
    for m in (-1e-9, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(MI355Error, match="min_std"):
            _norm(min_std=m)


def test_a_grown_gallery():
    norm = _norm("znorm", rows=5)
    gal = R.Gallery(8, "cpu")
    gal.rows = 5
    assert norm._check(gal) is gal
    gal.rows = 6                                                                   # as after add()
    for call in (lambda: norm._check(gal), lambda: norm.search(gal, torch.zeros(2, 8), 1), lambda: norm.scores(gal, torch.zeros(2, 8)),
                 lambda: norm.query_side(gal, torch.zeros(2, 8)), lambda: gal.search_normed(torch.zeros(2, 8), 1, norm)):
        with pytest.raises(MI355Error, match="fitted on 5 gallery rows, the gallery now holds 6"):
            call()
    with pytest.raises(MI355Error, match="not supported"):
        norm._check(M.Int8Gallery(8, "cpu"))
    with pytest.raises(MI355Error, match="must be a ScoreNorm"):
        gal.search_normed(torch.zeros(2, 8), 1, "csls")


def test_non_finite_coefficients():
    for bad in (float("nan"), float("inf"), -float("inf")):
        for name in ("ag", "bg"):
            t = torch.ones(5)
            t[3] = bad
            with pytest.raises(MI355Error, match=f"{name} has a non-finite coefficient"):
                _norm("znorm", **{name: t})
    with pytest.raises(MI355Error, match="bg has a non-finite"):
        _norm("csls", bg=torch.full((5,), float("nan")))


def test_wrong_lengths_dtypes_and_sides():
    for kw in (dict(ag=torch.ones(4)), dict(bg=torch.ones(6)), dict(ag=torch.ones(5, 1)), dict(ag=torch.ones(5, dtype=torch.float64)),
               dict(bg=torch.ones(5, dtype=torch.float16)), dict(bg=torch.ones(5, dtype=torch.int64)), dict(ag=[1.0] * 5)):
        with pytest.raises(MI355Error, match="must be|must have shape"):
            _norm("znorm", **kw)
    with pytest.raises(MI355Error, match='kind="csls" holds bg only'):
        S.ScoreNorm("csls", 5, ag=torch.ones(5), bg=torch.ones(5))
    with pytest.raises(MI355Error, match='kind="znorm" holds ag and bg'):
        S.ScoreNorm("znorm", 5, bg=torch.ones(5))
    with pytest.raises(MI355Error, match="no gallery side"):
        _norm("tnorm", ag=torch.ones(5))
    with pytest.raises(MI355Error, match="needs the cohort"):
        S.ScoreNorm("snorm", 5, ag=torch.ones(5), bg=torch.ones(5))
    with pytest.raises(MI355Error, match="rows"):
        S.ScoreNorm("znorm", 0, ag=torch.ones(0), bg=torch.ones(0))
    q, g = torch.zeros(6, 8), torch.zeros(20, 8)
    for kw, msg in ((dict(), "at least one of aq and ag"), (dict(bq=torch.ones(6)), "at least one of aq and ag"),
                    (dict(aq=torch.ones(5)), r"aq must have shape \(6,\)"), (dict(ag=torch.ones(6)), r"ag must have shape \(20,\)"),
                    (dict(aq=torch.ones(6), bg=torch.ones(20, dtype=torch.float64)), "bg must be float32"),
                    (dict(aq=torch.ones(6).tolist()), "aq must be None or a float32 tensor")):
        with pytest.raises(MI355Error, match=msg):
            M.adjusted_topk(q, g, 3, **kw)
        with pytest.raises(MI355Error, match=msg):
            M.adjusted_scores(q, g, **kw)
    ok = dict(aq=torch.ones(6))
    for k in (0, 21, 1.0, True):
        with pytest.raises(MI355Error, match="k out of range"):
            M.adjusted_topk(q, g, k, **ok)
    for qb in (-1, 1.0, True):
        with pytest.raises(MI355Error, match="query_block"):
            M.adjusted_topk(q, g, 3, query_block=qb, **ok)
    with pytest.raises(MI355Error, match="GPU"):                                  # every check passed: the device is next
        M.adjusted_topk(q, g, 3, **ok)
    with pytest.raises(MI355Error, match="not supported"):
        M.adjusted_topk(q, M.Int8Gallery(8, "cpu"), 3, **ok)


def test_where_the_public_names_live():
    for name in ("search_normed", "score_norm", "neighbourhood_stats"):
        assert name not in vars(M.Gallery) and callable(getattr(M.Gallery, name))
    assert R._ScoreNormed in M.Gallery.__bases__
    for name in ("ScoreNorm", "adjusted_topk", "adjusted_scores", "neighbourhood_stats"):
        assert name not in M.__all__ and getattr(M, name) is getattr(S, name)
    assert not hasattr(M.Int8Gallery, "search_normed") and not hasattr(M.ShardedGallery, "search_normed")
