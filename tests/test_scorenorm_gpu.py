"""Adjusted scores (CSLS, cohort normalisation) on the GPU against the NumPy model of tests/scorenorm_ref.py.

(a) Lattice rows (tests/rank_tiles_ref.py): every cosine is a multiple of 1 / 16 and every coefficient a small multiple of 1 / 8,
    so t = s * (aq + ag) - (bq + bg) is exact in any evaluation order and values and indices must equal the model element for
    element, in every loop family, for every fused list length (k = 1, 2, 3, 4, 5, 8), the slab (k = 9) and the bitonic selection
    (k = 150), unfiltered and filtered, with one launch and with a main and a tail launch, and with a caller's query block.
    Outputs and workspace hold 0xFF bytes before every call.
(b) Random rows: the adjusted slab is the model applied to the bits of ``cosine_scores``, the search is the model's top-k of that
    slab, and the first queries searched alone (the Q <= 4 path) return the same bits.
(c) The statistics kernel against the float64 model: count and mean bit for bit, the deviation and the coefficients within one
    fp32 ulp (the device's float64 square root and division are not shown here to round as NumPy's do).
(d) End to end on the planted-hub fixture: CSLS brings precision@1 from below 0.6 to above 0.9 and reproduces the model.
No tolerance appears in (a), (b) and (d)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import rank_tiles_ref as ref
import scorenorm_ref as SR
from imageretrievalresearch_amd import lib
from imageretrievalresearch_amd._lib import RankFilter, ScoreAdjust, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
F32 = np.float32
GEMV, SPLIT, EXACT, F16_GEMM, FUSED, BITONIC = 1, 2, 3, 5, 0x100, 0x200

# loop family -> (kind, D, raw rows (+-1, gallery_is_normalized = 0) or unit rows (+-0.25), MI355_RANK_EXACT_F32)
FAMILIES = {"split48": ("f32", 48, False, False), "split100raw": ("f32", 100, True, False), "exactvec48raw": ("f32", 48, True, True),
            "exact70": ("f32", 70, False, False), "f16-48": ("f16", 48, False, False), "f16-70": ("f16", 70, False, False),
            "f16-100": ("f16", 100, False, False)}
PATHS = {"split48": SPLIT, "split100raw": SPLIT, "exactvec48raw": EXACT, "exact70": EXACT, "f16-48": F16_GEMM, "f16-70": F16_GEMM,
         "f16-100": F16_GEMM}
QS, GS, KS = (1, 4, 5, 64, 65, 130, 300), (1, 127, 128, 129, 300), (1, 2, 3, 4, 5, 8, 9, 150)
SLOTS = 4               # the forced cut: six or nine tiles (two or three rows of query tiles) run a main and a tail launch


@pytest.fixture(autouse=True)
def _restore_the_override():
    yield
    assert lib().mi355_rank_set_round_slots(0) == 0


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _np(t):
    return t.cpu().numpy()


def _ok(status):
    assert status == 0, lib().mi355_last_error()


def _tiles():
    out = (C.c_int * 5)()
    assert lib().mi355_rank_last_tiles(out, 5) == 5
    return tuple(out)


def _env(monkeypatch, fam):
    if FAMILIES[fam][3]:
        monkeypatch.setenv("MI355_RANK_EXACT_F32", "1")
    else:
        monkeypatch.delenv("MI355_RANK_EXACT_F32", raising=False)


@functools.lru_cache(maxsize=None)
def _data(Q, G, D):
    """One lattice case: rows, labels, exclude, idx_offset (rank_tiles_ref.Data) and coefficients that are multiples of 1 / 8."""
    i = QS.index(Q) * len(GS) + GS.index(G)
    d = ref.Data(Q, G, D, 7000 + 10 * i + D, None, [ref.SAME, ref.DIFFERENT, ref.ANY][i % 3])
    rng = np.random.default_rng(99 + i)
    d.aq, d.ag = (rng.integers(1, 17, Q) / 8).astype(F32), (rng.integers(0, 9, G) / 8).astype(F32)
    d.bq, d.bg = (rng.integers(-8, 9, Q) / 8).astype(F32), (rng.integers(-8, 9, G) / 8).astype(F32)
    d.T = SR.adjust(ref.f32(d.S), d.aq, d.bq, d.ag, d.bg)
    exact = (d.S.astype(np.float64) / 16) * (d.aq.astype(np.float64)[:, None] + d.ag[None, :]) - (d.bq.astype(np.float64)[:, None] + d.bg[None, :])
    assert np.array_equal(d.T.astype(np.float64), exact)               # the premise: no step of the map rounds
    return d


class Inputs:
    """One lattice case on the device, as one loop family reads it."""

    def __init__(self, d, fam):
        self.d, self.fam = d, fam
        self.kind, D, self.raw, self.exact = FAMILIES[fam]
        self.q = torch.from_numpy(d.rows("q", self.raw)).to(DEV)
        g = torch.from_numpy(d.rows("g", self.raw)).to(DEV)
        self.keep = g
        if self.kind == "f16":
            self.keep = M.Gallery(D, DEV, dtype=torch.float16).add(g)
            self.g = self.keep._buf.data_ptr()
        else:
            self.g = g.data_ptr()
        self.norm = () if self.kind == "f16" else (0 if self.raw else 1,)
        self.sfx = "_f16" if self.kind == "f16" else ""
        self.ql, self.gl = torch.from_numpy(d.ql).to(DEV), torch.from_numpy(d.gl).to(DEV)
        self.excl = torch.from_numpy(d.excl).to(DEV)
        self.co = [torch.from_numpy(v).to(DEV) for v in (d.aq, d.bq, d.ag, d.bg)]
        self.adj = ScoreAdjust()
        self.adj.aq, self.adj.bq, self.adj.ag, self.adj.bg = (t.data_ptr() for t in self.co)
        self.filt = RankFilter()
        self.filt.label_mode = d.mode
        if d.mode != ref.ANY:
            self.filt.query_labels, self.filt.gallery_labels = self.ql.data_ptr(), self.gl.data_ptr()
        self.filt.exclude = self.excl.data_ptr()

    def _ws(self, k):
        n = int(getattr(lib(), "mi355_rank_adjusted%s_workspace_bytes" % self.sfx)(self.d.Q, self.d.G, self.d.D, k))
        assert n > 0
        return _poison((n + 4096,), torch.uint8), n

    def topk(self, k, filtered, slots=0, qblock=0):
        d, L = self.d, lib()
        ov, oi = _poison((d.Q, k), torch.float32), _poison((d.Q, k), torch.int64)
        w, n = self._ws(k)
        assert L.mi355_rank_set_round_slots(slots) == 0
        _ok(getattr(L, "mi355_rank_topk_adjusted" + self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, k, EPS, d.off,
                                                             C.byref(self.adj), C.byref(self.filt) if filtered else None, qblock,
                                                             ov.data_ptr(), oi.data_ptr(), w.data_ptr(), n, stream_ptr(DEV)))
        return (_np(ov), _np(oi)), L.mi355_rank_last_path(), _tiles()

    def slab(self, slots=0, qblock=0):
        d, L = self.d, lib()
        out = _poison((d.Q, d.G), torch.float32)
        w, n = self._ws(0)
        assert L.mi355_rank_set_round_slots(slots) == 0
        _ok(getattr(L, "mi355_cosine_scores_adjusted" + self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, EPS,
                                                                 C.byref(self.adj), qblock, out.data_ptr(), w.data_ptr(), n,
                                                                 stream_ptr(DEV)))
        return (_np(out),), L.mi355_rank_last_path(), _tiles()


def _variants(Q):
    """(slots, query_block) of every variant of a call: one launch; the forced cut where 128-query tiles run (Q > 64); the
    caller's query block at 300 queries (blocks of 128, 128 and 44: aq, bq and the filter shift twice)."""
    slots = 2 if Q <= 128 else SLOTS                              # (one row of query tiles: three column tiles are cut at two slots)
    return [(0, 0)] + ([(slots, 0)] if Q > 64 else []) + ([(0, 128), (slots, 128)] if Q == 300 else [])


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_lattice_rows_equal_the_model(fam, Q, G, monkeypatch):
    _env(monkeypatch, fam)
    d = _data(Q, G, FAMILIES[fam][1])
    x = Inputs(d, fam)
    for slots, qb in _variants(Q):
        got, path, tiles = x.slab(slots, qb)
        assert path == PATHS[fam], hex(path)                       # the tiles at every Q: no GEMV
        assert ref.same_result(got, (d.T,)), ("slab", slots, qb)
    cut = False
    for k in [k for k in KS if k <= G]:
        for filtered in (False, True):
            want = SR.topk(d.T, k, d.eligible(d.mode) if filtered else None, d.off)
            for slots, qb in _variants(Q):
                got, path, tiles = x.topk(k, filtered, slots, qb)
                fused = k <= 8 and Q > 4
                assert path == PATHS[fam] | (FUSED if fused else BITONIC if k > 8 else 0), (hex(path), k)
                assert ref.same_result(got, want), (k, filtered, slots, qb)
                cut = cut or (slots and tiles[2] > 0 and tiles[3] > 0)
    if Q > 64 and G == 300:
        assert cut                                                  # a main launch of 128-query tiles and a tail launch both ran


# ---------------------------------------------------------------- (b) random rows
def _scatter(vals, idx, G):
    out = torch.empty((vals.shape[0], G), dtype=torch.float32, device=vals.device)
    return out.scatter_(1, idx, vals)


@pytest.mark.parametrize("fam", ["split48", "exact70", "f16-48", "f16-70"])
def test_random_rows_equal_the_model_applied_to_cosine_scores(fam, monkeypatch):
    _env(monkeypatch, fam)
    kind, D = FAMILIES[fam][:2]
    Q, G = 7, 300
    gen = torch.Generator().manual_seed(31 + D)
    q, g = torch.randn((Q, D), generator=gen).to(DEV), torch.randn((G, D), generator=gen).to(DEV)
    co = dict(aq=torch.rand(Q, generator=gen) + 0.5, bq=torch.randn(Q, generator=gen), ag=torch.rand(G, generator=gen),
              bg=torch.randn(G, generator=gen))
    co = {k: v.to(DEV) for k, v in co.items()}
    if kind == "f16":
        gal = M.Gallery(D, DEV, dtype=torch.float16).add(g)
        S = _np(_scatter(*gal.search(q, G), G))                    # fp16 rows have no slab entry: every score of the k = G search
    else:
        gal = g
        S = _np(M.cosine_scores(q, g))
    for drop in ((), ("aq", "bq"), ("ag", "bg"), ("aq",), ("bq",), ("ag",), ("bg",)):
        use = {k: v for k, v in co.items() if k not in drop}
        T = SR.adjust(S, **{k: _np(v) for k, v in use.items()})
        assert ref.same_result((_np(M.adjusted_scores(q, gal, **use)),), (T,)), drop
        for k in (3, 9):
            got = M.adjusted_topk(q, gal, k, **use, idx_offset=11)
            assert ref.same_result((_np(got[0]), _np(got[1])), SR.topk(T, k, None, 11)), (drop, k)
            first = {n: (v[:3] if n in ("aq", "bq") else v) for n, v in use.items()}
            alone = M.adjusted_topk(q[:3], gal, k, **first, idx_offset=11)   # Q <= 4: the adjusted slab on the tiles
            assert ref.same_result((_np(alone[0]), _np(alone[1])), (_np(got[0])[:3], _np(got[1])[:3])), (drop, k)
        assert ref.same_result((_np(M.adjusted_scores(q[:3], gal, **first)),), (T[:3],)), drop


# ---------------------------------------------------------------- (c) the statistics kernel
def _ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("N,n", [(67, 13), (5, 1), (3, 1024), (300, 10)])
def test_statistics_against_the_float64_model(N, n):
    rng = np.random.default_rng(N * 1000 + n)
    vals = -np.sort(-rng.uniform(-1, 1, (N, n)).astype(F32), axis=1)
    idx = rng.integers(0, 5000, (N, n)).astype(np.int64)
    for r in range(0, N, 3):                                       # pads at the tail, as a filtered search leaves them
        p = int(rng.integers(0, n + 1))
        vals[r, n - p:], idx[r, n - p:] = -np.inf, -1
    vals[N // 2], idx[N // 2] = -np.inf, -1                         # a row with no eligible entry
    if N > 4:
        vals[1] = vals[1, 0]                                        # a constant row: deviation 0, the floor
    tv, ti = torch.from_numpy(vals).to(DEV), torch.from_numpy(idx).to(DEV)
    for half, min_std in ((None, 1e-6), (1.0, 1e-6), (0.5, 1e-3)):
        got = [_np(t) for t in M.topn_stats(tv, ti, half, min_std)]
        want = SR.topn_stats(vals, idx, half, min_std)
        assert len(got) == len(want)
        assert np.array_equal(got[2], want[2]) and got[2].dtype == np.int32
        assert ref.same_result((got[0],), (want[0],))               # the mean: bit for bit
        assert got[2][N // 2] == 0 and got[0][N // 2] == 0 and got[1][N // 2] == 0
        worst = [int(_ulps(g, w).max()) for g, w in zip(got[1:2] + got[3:], want[1:2] + want[3:])]
        print(f"N={N} n={n} half={half}: std / a / b differ from the float64 model by at most {worst} fp32 ulp")
        assert max(worst) <= 1


# ---------------------------------------------------------------- (d) end to end on the planted hubs
def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the fixture's arrays are read-only)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_csls_removes_the_hubs_and_reproduces_the_model(dtype):
    f = SR.hub_fixture(0)
    q, c, ql = _dev(f["queries"]), _dev(f["cohort"]), _dev(f["query_labels"])
    G = f["gallery"].shape[0]
    gal = M.Gallery(64, DEV, dtype=dtype).add(_dev(f["gallery"]), _dev(f["gallery_labels"]))
    cn = M.l2_normalize_rows(c)
    # the library's own cosine bits, from entry points that existed before: the model does the rest
    Sgc = _np(M.cosine_scores(gal.data.float(), cn, gallery_is_normalized=True))
    Sqc = _np(M.cosine_scores(q, cn, gallery_is_normalized=True))
    Sqg = _np(_scatter(*gal.search(q, G), G))
    plain = _np(gal.search(q, 1)[1])
    p_plain = SR.precision_at_1(plain, f["query_labels"], f["gallery_labels"])
    norm = gal.score_norm(c, "csls")
    assert norm.n == 10 and norm.ag is None
    aq, bq, ag, bg = SR.coefficients("csls", Sgc, Sqg, Sqc)
    assert ref.same_result((_np(norm.bg),), (bg,))
    T = SR.adjust(Sqg, aq, bq, ag, bg)
    for k in (1, 3, 10):
        got = gal.search_normed(q, k, norm)
        assert ref.same_result((_np(got[0]), _np(got[1])), SR.topk(T, k))
    assert ref.same_result((_np(norm.scores(gal, q)),), (T,))
    p_csls = SR.precision_at_1(_np(gal.search_normed(q, 1, norm)[1]), f["query_labels"], f["gallery_labels"])
    print(f"{dtype}: precision@1 plain {p_plain:.3f}, CSLS {p_csls:.3f}")
    assert p_plain < 0.6 and p_csls > 0.9
    # the filter arguments reach both the query's neighbourhood and the search
    elig = f["query_labels"][:, None] != f["gallery_labels"][None, :]
    co = SR.coefficients("csls", Sgc, Sqg, Sqc, elig=elig)
    got = gal.search_normed(q, 3, norm, 5, query_labels=ql, label_filter="different")
    assert ref.same_result((_np(got[0]), _np(got[1])), SR.topk(SR.adjust(Sqg, *co), 3, elig, 5))
    # the norms: search_normed is adjusted_topk with the norm's own vectors, and those are the model's within an ulp
    for kind, n in (("znorm", None), ("tnorm", None), ("snorm", 40)):
        nz = gal.score_norm(c, kind, n)
        vq = nz.query_side(gal, q)
        got = gal.search_normed(q, 3, nz)
        low = M.adjusted_topk(q, gal, 3, aq=vq[0], bq=vq[1], ag=nz.ag, bg=nz.bg)
        assert ref.same_result((_np(got[0]), _np(got[1])), (_np(low[0]), _np(low[1]))), kind
        want = SR.coefficients(kind, Sgc, Sqg, Sqc, n)
        for name, g_, w_ in zip(("aq", "bq", "ag", "bg"), vq + (nz.ag, nz.bg), want):
            assert (g_ is None) == (w_ is None), (kind, name)
            if g_ is not None:
                assert _ulps(_np(g_), w_).max() <= 1, (kind, name)
    if dtype == torch.float32:                                      # a prepared gallery is searched on its fp32 rows: same bits
        prep = M.Gallery(64, DEV).add(_dev(f["gallery"]), _dev(f["gallery_labels"])).prepare()
        pn = prep.score_norm(c, "csls")
        assert ref.same_result((_np(pn.bg),), (bg,))
        got = prep.search_normed(q, 3, pn)
        assert ref.same_result((_np(got[0]), _np(got[1])), SR.topk(T, 3))
    gal.add(_dev(f["gallery"][:2]))
    with pytest.raises(M.MI355Error, match="fit again"):
        gal.search_normed(q, 3, norm)
