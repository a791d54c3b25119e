"""The row norm and the row-wise ops on the GPU against their float64 definitions (tests/rowops_ref.py), within the error bounds
derived there: ``l2_normalize_rows`` on both load paths of ``row_inv_norm`` (float4 loads of 16-byte aligned rows, scalar loads
otherwise - reached here with dim % 4 == 0 through a contiguous view that starts 4 bytes into its buffer), the galleries and
the cosine entry points on such a view, ``pair_cosine``, ``ContrastiveLoss`` and ``CosineEmbeddingLoss`` at the edges of their
row and lane loops, and ``synth_fill`` past one trip of its grid-stride loop.  Every test prints its observed maximum error in
units of its bound (pytest -s)."""
import numpy as np
import pytest
import torch

import binary_ref
import gallery_fp4_ref
import gallery_i8_ref
import kmeans_ref
import qe_ref
import rowops_ref as R
import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import Int8Gallery, MI355Error, binary, synth
from imageretrievalresearch_amd._lib import check, lib, stream_ptr
from imageretrievalresearch_amd.fp4 import FP4Gallery

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_GEMV, PATH_SPLIT, PATH_EXACT_F32 = 1, 2, 3                    # MI355_RANK_PATH_* of include/mi355_retrieval.h


def dev(x):
    t = (x.clone() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def offset_view(x):
    """The values of x (numpy or tensor) as a contiguous tensor that starts 4 bytes into a 16-byte aligned buffer."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = flat[1: 1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.dtype == torch.float32 and v.data_ptr() % 16 == 4
    return v


PLACE = {"aligned": dev, "offset": offset_view}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _units(err, bound):
    """max err / bound over the entries with a positive bound; an entry with bound 0 must be exact."""
    err, bound = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _rel(got, ref):
    """max |got - ref| / |ref| (ref without zeros)."""
    return float((np.abs(_np(got).astype(np.float64) - ref) / np.abs(ref)).max())


# ------------------------------------------------------------------------------------------------ l2_normalize_rows
@pytest.mark.parametrize("dim", R.NORM_DIMS)
def test_l2_normalize_rows_against_float64_on_both_load_paths(dim):
    bound, worst = R.normalize_bound(dim), {}
    for rows in R.NORM_ROWS:
        x = R.norm_case(rows, dim)
        ref = R.normalize(x)
        for how, place in PLACE.items():                             # dim % 4 == 0: float4 loads / scalar loads
            t = place(x)
            got = M.l2_normalize_rows(t)
            assert got.shape == (rows, dim) and got.dtype == torch.float32 and got.data_ptr() != t.data_ptr()
            rel = _rel(got, ref)
            worst[how] = max(worst.get(how, 0.0), rel)
            assert rel <= bound, (dim, rows, how, rel / R.U)
    print(f"dim={dim}: max relative error " + ", ".join(f"{h} {w / R.U:.2f} U = {w / bound:.3f} of the bound" for h, w in worst.items()))


@pytest.mark.parametrize("how", list(PLACE))
@pytest.mark.parametrize("dim", [256, 255])
def test_l2_normalize_rows_edge_rows(dim, how):
    rng = np.random.default_rng(dim)
    clean = rng.standard_normal((9, dim)).astype(np.float32)        # norms about 16
    clean[0] = 0.0                                                   # a zero row
    clean[1] *= np.float32(1e-9 / 16)                                # norm about 1e-9, below eps
    clean[2] *= np.float32(1e-15)
    clean[3] *= np.float32(1e15)
    x = clean.copy()
    x[5, 7], x[5, dim - 2] = np.nan, np.inf                          # rows 4 ... 7 share a block
    x[8, dim // 2] = -np.inf
    place = PLACE[how]
    got, got_clean = M.l2_normalize_rows(place(x)), M.l2_normalize_rows(place(clean))
    g, ref = _np(got), R.normalize(clean)
    e32 = float(np.float32(R.EPS))
    assert (g[0] == 0).all()
    for r in (1, 2):                                                 # below eps: x / eps, two roundings
        assert _rel(got_clean[r], clean[r].astype(np.float64) / e32) <= 2 * R.U
    live = [3, 4, 6, 7]
    assert _rel(got_clean[live], ref[live]) <= R.normalize_bound(dim)
    assert np.isnan(g[5]).all()                                      # a NaN element (and an Inf): the whole row
    assert torch.equal(_bits(got[[4, 6, 7]]), _bits(got_clean[[4, 6, 7]]))      # its block neighbours: untouched
    assert torch.equal(_bits(got[:4]), _bits(got_clean[:4]))
    inf_at = np.arange(dim) == dim // 2                              # an Inf alone: x / inf = 0, inf / inf = NaN
    assert np.isnan(g[8][inf_at]).all() and (g[8][~inf_at] == 0).all()
    # other eps: 1e-30 normalises the tiny rows too, 20 clamps every row of norm 16
    tiny = M.l2_normalize_rows(place(clean), eps=1e-30)
    assert _rel(tiny[1:], R.normalize(clean[1:], 1e-30)) <= R.normalize_bound(dim)
    big = M.l2_normalize_rows(place(clean), eps=20.0)
    want = R.normalize(clean, 20.0)
    assert np.abs(np.sqrt((want[4:] ** 2).sum(1)) - 0.8).max() < 0.1 and abs(np.sqrt((want[3] ** 2).sum()) - 1) < 1e-9
    assert _rel(big[1:], want[1:]) <= R.normalize_bound(dim) and (_np(big[0]) == 0).all()
    # in place, and twice
    y = place(x)
    assert M.l2_normalize_rows(y, out=y) is y
    assert torch.equal(_bits(y), _bits(got))
    assert torch.equal(_bits(M.l2_normalize_rows(place(x))), _bits(got))


def test_l2_normalize_rows_checks_out():
    x = dev(R.norm_case(5, 64))
    want = M.l2_normalize_rows(x)
    out = torch.full((5, 64), 7.0, device=DEV)
    assert M.l2_normalize_rows(x, out=out) is out and torch.equal(out, want)
    view = offset_view(torch.zeros(5, 64))
    assert M.l2_normalize_rows(x, out=view) is view and _rel(view, R.normalize(_np(x))) <= R.normalize_bound(64)
    wide = torch.zeros((5, 128), device=DEV)
    for bad in (torch.zeros((5, 65), device=DEV), torch.zeros((6, 64), device=DEV), torch.zeros((64, 5), device=DEV),
                torch.zeros(5 * 64, device=DEV), torch.zeros((5, 64), device=DEV, dtype=torch.float16),
                torch.zeros((5, 64), device=DEV, dtype=torch.float64), torch.zeros((5, 64)), wide[:, :64],
                torch.zeros((64, 5), device=DEV).t(), np.zeros((5, 64), np.float32)):
        with pytest.raises(MI355Error, match="out must be a contiguous float32"):
            M.l2_normalize_rows(x, out=bad)
    assert (wide == 0).all()


# ------------------------------------------------------------------------------------------------ the galleries on a view
@pytest.mark.parametrize("D", [256, 1536])
def test_galleries_follow_the_rule_on_an_unaligned_source(D):
    """Every conversion takes the norm as l2_normalize_rows takes it for the same pointer: scalar loads here."""
    view = offset_view(R.norm_case(9, D))
    n = M.l2_normalize_rows(view)
    assert _rel(n, R.normalize(_np(view))) <= R.normalize_bound(D)
    half = M.Gallery(D, DEV, dtype=torch.float16).add(view)
    assert torch.equal(half.data.view(torch.int16), n.half().view(torch.int16))
    assert torch.equal(_bits(M.Gallery(D, DEV).add(view).data), _bits(n))
    i8 = Int8Gallery(D, DEV).add(view)
    codes, scales = gallery_i8_ref.quantize_rows(_np(n))
    assert (_np(i8.codes) == codes).all() and (_np(i8.scales).view(np.int32) == scales.astype(np.float32).view(np.int32)).all()
    f4 = FP4Gallery(D, DEV).add(view)
    codes, mults = gallery_fp4_ref.quantize_rows(_np(n))
    assert (_np(f4.codes) == gallery_fp4_ref.pack(codes)[:, : (D + 1) // 2]).all()
    assert (_np(f4.mults).view(np.int32) == mults.astype(np.float32).view(np.int32)).all()
    b = binary.BinaryGallery(D, DEV).add(view)
    assert (np.ascontiguousarray(_np(b.codes)).view(np.uint32) == binary_ref.encode(_np(n))).all()


# ------------------------------------------------------------------------------------------------ the cosine entry points
def _base_path():
    return lib().mi355_rank_last_path() & 0xff


def _assert_topk(v, i, s64, k, what):
    order, srt, cert = R.topk64(s64, k)
    assert (~cert).sum() <= 0.1 * len(s64), what
    err = float(np.abs(_np(v).astype(np.float64) - srt[:, :k]).max())
    assert err <= R.SCORE_BOUND, (what, err)
    assert (_np(i)[cert] == order[cert][:, :k]).all(), what
    return err


@pytest.mark.parametrize("side", ["gallery", "queries"])
@pytest.mark.parametrize("Q", R.COSINE_QS)
def test_cosine_entry_points_on_unaligned_operands(Q, side, monkeypatch):
    """D = 256, G = 300: the operand named by ``side`` is the 4-byte-offset view, the other one is aligned.  An unaligned
    gallery takes the exact-fp32 tiles (the GEMV where an entry has one and Q <= 4), unaligned queries leave the split."""
    monkeypatch.delenv("MI355_RANK_EXACT_F32", raising=False)
    q, g = R.cosine_case(Q)
    G, D = g.shape
    tq = offset_view(q) if side == "queries" else dev(q)
    put_g = offset_view if side == "gallery" else dev
    tg = put_g(g)
    gn = M.l2_normalize_rows(dev(g))                                 # a stored unit gallery, then placed like g
    tgn, gn64 = put_g(gn), _np(gn).astype(np.float64)
    tiles = PATH_EXACT_F32 if side == "gallery" else PATH_SPLIT
    gemv = PATH_GEMV if Q <= 4 else tiles
    s64, s64n = R.cosine64(q, g), R.cosine64(q, gn64, unit_gallery=True)
    worst = {}

    S = M.cosine_scores(tq, tg)
    assert _base_path() == gemv
    worst["scores"] = float(np.abs(_np(S).astype(np.float64) - s64).max())
    Sn = M.cosine_scores(tq, tgn, gallery_is_normalized=True)
    assert _base_path() == gemv
    worst["scores unit"] = float(np.abs(_np(Sn).astype(np.float64) - s64n).max())
    assert max(worst.values()) <= R.SCORE_BOUND, worst

    for k in R.COSINE_KS:
        v, i = M.cosine_topk(tq, tg, k)
        assert _base_path() == gemv
        worst[f"topk {k}"] = _assert_topk(v, i, s64, k, f"raw k={k}")
        v, i = M.cosine_topk(tq, tgn, k, gallery_is_normalized=True)
        assert _base_path() == gemv
        worst[f"topk {k} unit"] = _assert_topk(v, i, s64n, k, f"unit k={k}")

    t = 0.5
    res = M.cosine_range(tq, tg, t)
    assert _base_path() == tiles                                     # any Q: the tiled GEMM
    off, idx, sc = _np(res.offsets), _np(res.indices), _np(res.scores).astype(np.float64)
    hit = np.zeros((Q, G), bool)
    rows = np.repeat(np.arange(Q), np.diff(off))
    hit[rows, idx] = True
    assert hit.sum() == len(idx) > 0 and all((np.diff(idx[off[r]: off[r + 1]]) > 0).all() for r in range(Q))
    assert hit[s64 >= t + R.SCORE_BOUND].all() and not hit[s64 <= t - R.SCORE_BOUND].any()
    worst["range"] = float(np.abs(sc - s64[rows, idx]).max())
    assert worst["range"] <= R.SCORE_BOUND

    # assign_clusters(rows = the gallery, centroids = the queries), with the conditions of tests/test_kmeans_gpu.py
    a, s = M.assign_clusters(tg, tq)
    assert _base_path() == tiles
    a, s = _np(a), _np(s).astype(np.float64)
    ra, _, gap = kmeans_ref.assign(g, q)
    chosen = s64.T[np.arange(G), a]
    assert (s64.T.max(axis=1) - chosen).max() <= 2e-5 and np.abs(s - chosen).max() <= 1e-5
    assert (gap >= 1e-4).mean() >= 0.9 and (a[gap >= 1e-4] == ra[gap >= 1e-4]).all()
    worst["assign"] = float(np.abs(s - chosen).max())

    # expand_queries, with the tolerance of tests/test_query_expansion_gpu.py (n = 5: 4e-6 per row, where round 1 is certified)
    n, alpha = 5, 3.0
    for unit, gal, rows64 in ((False, tg, qe_ref.normalize(g)), (True, tgn, gn64)):
        out = M.expand_queries(tq, gal, n, alpha, gallery_is_normalized=unit)
        assert _base_path() == (PATH_GEMV if Q <= 4 else tiles)     # round 1 is a top-k search
        S1 = qe_ref.normalize(q) @ rows64.T
        order = np.argsort(-S1, axis=1, kind="stable")[:, :n]
        want = qe_ref.expand(q, rows64, np.take_along_axis(S1, order, 1), order, alpha)
        cert = qe_ref.gaps(S1, n) > 5e-5
        assert cert.mean() > 0.5
        err = np.sqrt(((_np(out).astype(np.float64) - want) ** 2).sum(1))[cert].max()
        assert err <= max(4e-6, (n + 2) * 2.0 ** -23), (unit, err)
        worst["expand unit" if unit else "expand"] = float(err)
    print(f"Q={Q}, unaligned {side}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ pair_cosine
def _placings(dim):
    """How the two operands are placed: aligned, and at dim 256 also one or both 4 bytes off."""
    return [(dev, dev)] + ([(offset_view, dev), (offset_view, offset_view)] if dim == 256 else [])


@pytest.mark.parametrize("dim", R.OP_DIMS)
def test_pair_cosine_against_float64(dim):
    worst = 0.0
    for rows in R.PAIR_ROWS:
        a, b = R.pair_case(rows, dim)
        ref, bound = R.pair_cosine(a, b), R.pair_cosine_bound(a, b)
        for pa, pb in _placings(dim):
            got = M.pair_cosine(pa(a), pb(b))
            assert got.shape == (rows,) and got.dtype == torch.float32
            u = _units(np.abs(_np(got).astype(np.float64) - ref), bound)
            worst = max(worst, u)
            assert u <= 1.0, (dim, rows, u)
    print(f"dim={dim}: max error {worst:.3f} of the bound")


def test_pair_cosine_edge_rows():
    a, b = R.pair_case(9, 65)
    a[0], b[0] = 0.0, 0.0                                            # both zero: 0 / (eps eps) = 0, not NaN
    a[1] = 0.0                                                       # one zero
    a[2] *= np.float32(1e-9) / np.float32(np.sqrt((a[2].astype(np.float64) ** 2).sum()))     # |a| below eps, |b| above: the
    clean_a = a.copy()                                               # clamp applies to each norm on its own
    a[5, 64] = np.nan                                                # the tail lane of a row in the second block
    got, clean = _np(M.pair_cosine(dev(a), dev(b))), _np(M.pair_cosine(dev(clean_a), dev(b)))
    assert got[0] == 0 and got[1] == 0 and np.isnan(got[5])
    keep = np.arange(9) != 5
    assert (got[keep].view(np.int32) == clean[keep].view(np.int32)).all()
    ref, bound = R.pair_cosine(clean_a, b), R.pair_cosine_bound(clean_a, b)
    assert abs(ref[2]) > 1e-5 and abs(ref[2]) < 2e-3                 # (|a| / eps) cos: the unclamped cosine would be ~0.1 ... 1
    assert _units(np.abs(clean.astype(np.float64) - ref), bound) <= 1.0
    # another eps: both norms clamped
    got = _np(M.pair_cosine(dev(clean_a), dev(b), eps=1e3)).astype(np.float64)
    assert _units(np.abs(got - R.pair_cosine(clean_a, b, 1e3)), R.pair_cosine_bound(clean_a, b, 1e3)) <= 1.0


# ------------------------------------------------------------------------------------------------ ContrastiveLoss
def _contrastive_rows(a, b, label, margin, mean):
    """mi355_contrastive_loss with a per-row buffer of rows + 1 floats: (loss, per-row losses, the sentinel)."""
    rows, dim = a.shape
    out = torch.empty((), dtype=torch.float32, device=DEV)
    per = torch.full((rows + 1,), -7.0, dtype=torch.float32, device=DEV)
    with torch.cuda.device(a.device):
        check(lib().mi355_contrastive_loss(a.data_ptr(), b.data_ptr(), rows, dim, float(label), float(margin), int(mean),
                                           out.data_ptr(), per.data_ptr(), stream_ptr(a.device)))
    per = _np(per)
    return out, per[:rows], per[rows]


@pytest.mark.parametrize("dim", R.OP_DIMS)
def test_contrastive_loss_against_float64(dim):
    worst = 0.0
    for rows in R.LOSS_ROWS:
        f1, f2 = R.contrastive_case(rows, dim)
        for p1, p2 in _placings(dim):
            a, b = p1(f1), p2(f2)
            for label in R.CL_LABELS:
                for margin in R.CL_MARGINS:
                    ref, bound = R.contrastive(f1, f2, label, margin), R.contrastive_bound(f1, f2, label, margin)
                    for mean in (True, False):
                        got = M.ContrastiveLoss(margin)(a, b, label, mean)
                        assert got.shape == () and got.dtype == torch.float32
                        u = _units(abs(got.item() - ref[2 if mean else 1]), bound[2 if mean else 1])
                        worst = max(worst, u)
                        assert u <= 1.0, (dim, rows, label, margin, mean, u)
                    out, per, sentinel = _contrastive_rows(a, b, label, margin, True)
                    assert sentinel == -7.0 and torch.equal(_bits(out), _bits(M.ContrastiveLoss(margin)(a, b, label, True)))
                    u = _units(np.abs(per.astype(np.float64) - ref[0]), bound[0])
                    worst = max(worst, u)
                    assert u <= 1.0, (dim, rows, label, margin, "per row", u)
    print(f"dim={dim}: max error {worst:.3f} of the bound")


def test_contrastive_loss_of_identical_inputs():
    f1, _ = R.contrastive_case(17, 65)
    a = dev(f1)
    for label in R.CL_LABELS:
        for margin in R.CL_MARGINS:
            ref, bound = R.contrastive(f1, f1, label, margin), R.contrastive_bound(f1, f1, label, margin)
            out, per, sentinel = _contrastive_rows(a, a, label, margin, False)
            assert sentinel == -7.0 and (per == per[0]).all()
            assert _units(np.abs(per.astype(np.float64) - ref[0]), bound[0]) <= 1.0
            assert _units(abs(out.item() - ref[1]), bound[1]) <= 1.0
            if margin == 0.0 or label == 1.0:
                assert out.item() == 0.0                             # d = 0 and no hinge: exactly zero


# ------------------------------------------------------------------------------------------------ CosineEmbeddingLoss
@pytest.mark.parametrize("dim", R.OP_DIMS)
def test_cosine_embedding_loss_against_float64(dim):
    worst = 0.0
    for rows in R.LOSS_ROWS:
        x1, x2 = R.pair_case(rows, dim)
        x1[0] = 0.0                                                  # a zero row: cos = 0, not NaN
        for p1, p2 in _placings(dim):
            a, b = p1(x1), p2(x2)
            for target in R.CE_TARGETS:
                for margin in R.CE_MARGINS:
                    ref, bound = R.cosine_embedding(x1, x2, target, margin), R.cosine_embedding_bound(x1, x2, target, margin)
                    for reduction, pick in (("mean", 2), ("sum", 1)):
                        loss = M.CosineEmbeddingLoss(margin, reduction)
                        got = loss(a, b, target)
                        assert got.shape == () and got.dtype == torch.float32 and np.isfinite(got.item())
                        assert torch.equal(_bits(got), _bits(loss(a, b, torch.tensor([target]))))    # labels["pos"] / ["neg"]
                        u = _units(abs(got.item() - ref[pick]), bound[pick])
                        worst = max(worst, u)
                        assert u <= 1.0, (dim, rows, target, margin, reduction, u)
    print(f"dim={dim}: max error {worst:.3f} of the bound")


def test_cosine_embedding_loss_rejects_a_target_per_row():
    a, b = (dev(x) for x in R.pair_case(3, 64))
    with pytest.raises(MI355Error, match="scalar"):
        M.CosineEmbeddingLoss()(a, b, torch.tensor([1.0, -1.0, 1.0]))
    with pytest.raises(MI355Error):
        M.CosineEmbeddingLoss()(a, b, 0.5)                           # neither +1 nor -1


# ------------------------------------------------------------------------------------------------ synth_fill
@pytest.mark.parametrize("kind", [synth.UNIFORM, synth.NORMAL])
def test_synth_fill_second_trip_and_an_offset_past_2_to_32(kind):
    """2048 x 256 threads: n = 2048 * 256 + 77 sends 77 threads round the grid-stride loop again; the offset needs 64 bits."""
    n, seed, off = 2048 * 256 + 77, 91, 2 ** 33 + 5
    got = M.synth_fill(n, seed, kind, DEV, offset=off).cpu().numpy()
    want = synth.fill(seed, n, kind, offset=off)
    assert (got.view(np.int32) == want.view(np.int32)).all()
    assert (want[-77:] != synth.fill(seed, 77, kind, offset=5 + 2048 * 256)).any()      # (the high offset bits matter)
    one = M.synth_fill(1, seed, kind, DEV, offset=off + n - 1).cpu().numpy()
    assert one.shape == (1,) and one.view(np.int32)[0] == want.view(np.int32)[-1]
    assert M.synth_fill(0, seed, kind, DEV, offset=off).shape == (0,)
