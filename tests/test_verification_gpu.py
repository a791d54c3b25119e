"""Verification ROC on the GPU: roc_curve against a float64 restatement of utils/roc_curve_from_scratch.py on its data file,
float32 rounding boundaries, all-pairs counts exactly equal to counting the materialised cosine_scores slab on the same
path (asserting the path), the fp16 gallery, a 100k x 100k same-source call, edge cases, and the sharded histogram
(2 and 3 gloo ranks on one GPU).  The float64 references live here."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPLIT, EXACT, F16_GEMM = 2, 3, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binary_preds.csv")
GRID = np.array(list(range(0, 105, 5))) / 100


def _randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


def _labels(n, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, classes, (n,), generator=g).to(DEV)


def _trapz(y, x):
    return (getattr(np, "trapezoid", None) or np.trapz)(y, x)


def _bins(scores, thr):
    """Number of thresholds t with score >= t compared in float64 (NaN: 0)."""
    t = torch.as_tensor(np.asarray(thr, dtype=np.float64), device=scores.device)
    s = scores.double()
    b = torch.searchsorted(t, s.contiguous(), right=True)
    return torch.where(torch.isnan(s), torch.zeros_like(b), b)


def _hist_of(scores, gen, valid, thr):
    b = _bins(scores, thr)
    T = len(thr)
    return torch.stack([torch.bincount(b[valid & gen], minlength=T + 1), torch.bincount(b[valid & ~gen], minlength=T + 1)])


def _counts_from_hist(h):
    sg = h[0].flip(0).cumsum(0).flip(0)[1:]
    si = h[1].flip(0).cumsum(0).flip(0)[1:]
    ng, ni = h[0].sum(), h[1].sum()
    return {"tp": sg, "fp": si, "fn": ng - sg, "tn": ni - si, "num_genuine": ng, "num_impostor": ni}


def _assert_counts(r, h):
    want = _counts_from_hist(h.to(DEV))
    for key, v in want.items():
        assert torch.equal(r[key].to(torch.int64), v.to(torch.int64)), key
    with np.errstate(invalid="ignore"):            # (numpy's true division; 0 / 0 = NaN)
        tpr = want["tp"].cpu().numpy() / np.float64(int(want["num_genuine"]))
        fpr = want["fp"].cpu().numpy() / np.float64(int(want["num_impostor"]))
    assert np.array_equal(r["tpr"].cpu().numpy(), tpr, equal_nan=True)
    assert np.array_equal(r["fpr"].cpu().numpy(), fpr, equal_nan=True)
    if not np.isnan(tpr).any() and not np.isnan(fpr).any():
        assert abs(float(r["auc"]) - abs(_trapz(tpr, fpr))) < 1e-12


# ---------------------------------------------------------------- 1. golden: the reference script's data file
def _reference_recipe(actual, pred, thresholds):
    rows = []
    for t in thresholds:
        pc = pred >= t
        tp = int(np.sum(pc & (actual == 1)))
        fn = int(np.sum(~pc & (actual == 1)))
        fp = int(np.sum(pc & (actual == 0)))
        tn = int(np.sum(~pc & (actual == 0)))
        rows.append((tp, fp, fn, tn))
    c = np.array(rows)
    tpr = c[:, 0] / (c[:, 0] + c[:, 2])
    fpr = c[:, 1] / (c[:, 3] + c[:, 1])
    return c, tpr, fpr, abs(_trapz(tpr, fpr))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_golden_binary_preds(dtype):
    data = np.loadtxt(GOLDEN, delimiter=",", skiprows=1)
    actual, pred = data[:, 0], data[:, 1]
    assert pred.shape == (5696,)
    assert np.array_equal(pred.astype(np.float32).astype(np.float64), pred)       # the predictions are exact float32 values
    c, tpr, fpr, auc = _reference_recipe(actual, pred, GRID)
    r = M.roc_curve(torch.from_numpy(pred).to(DEV, dtype), torch.from_numpy(actual).to(DEV))
    got = torch.stack([r["tp"], r["fp"], r["fn"], r["tn"]], 1).cpu().numpy()
    assert np.array_equal(got, c)
    assert int(r["num_genuine"]) == 2848 and int(r["num_impostor"]) == 2848
    assert [int(r["tp"][i]) for i in (0, 10, 20)] == [2848, 2789, 0]
    assert [int(r["fp"][i]) for i in (0, 10, 20)] == [2792, 52, 0]
    assert np.array_equal(r["tpr"].cpu().numpy(), tpr) and np.array_equal(r["fpr"].cpu().numpy(), fpr)
    assert abs(float(r["auc"]) - auc) < 1e-12
    assert round(float(r["auc"]), 4) == 0.9776
    assert np.array_equal(r["thresholds"].cpu().numpy(), GRID)


def test_other_class_codes_count_in_neither_class():
    s = torch.tensor([0.1, 0.6, 0.9, 0.3, 0.7], device=DEV)
    a = torch.tensor([1.0, 0.0, 2.0, 0.5, 1.0], device=DEV)
    r = M.roc_curve(s, a)
    assert int(r["num_genuine"]) == 2 and int(r["num_impostor"]) == 1
    assert int(r["tp"][10]) == 1 and int(r["fp"][10]) == 1


# ---------------------------------------------------------------- 2. float32 rounding boundaries
def _ceil32(t):
    f = np.float32(t)
    return f if float(f) >= t else np.nextafter(f, np.float32(np.inf))


@pytest.mark.parametrize("thr", [GRID, np.array([-0.7, 0.1, 1 / 3, 0.35, 0.45, 0.65, 0.7, 0.9, 0.95])], ids=["grid", "mixed"])
def test_rounding_boundaries(thr):
    assert all(float(np.float32(t)) < t for t in (0.35, 0.45, 0.65, 0.7, 0.9, 0.95))     # they round DOWN to float32
    vals = []
    for t in thr:
        f = _ceil32(t)
        vals += [f, np.nextafter(f, np.float32(-np.inf)), np.float32(t), np.nextafter(f, np.float32(np.inf))]
    s32 = np.array(vals, dtype=np.float32)
    s32 = np.concatenate([s32, s32])
    act = np.concatenate([np.ones(len(vals)), np.zeros(len(vals))])
    for s in (torch.from_numpy(s32).to(DEV), torch.from_numpy(s32.astype(np.float64)).to(DEV)):
        r = M.roc_curve(s, torch.from_numpy(act).to(DEV), thresholds=thr)
        for i, t in enumerate(thr):
            p = s32.astype(np.float64) >= t
            assert int(r["tp"][i]) == int(np.sum(p & (act == 1))), (t, s.dtype)
            assert int(r["fp"][i]) == int(np.sum(p & (act == 0))), (t, s.dtype)


# ---------------------------------------------------------------- 3. all pairs: exactly the counts of the materialised slab
def _grid(kind):
    if kind == "t1":
        return np.array([0.05])
    if kind == "t21":
        return GRID
    if kind == "t4096":
        return np.linspace(-1.0, 1.0, 4096)
    r = np.sort(np.random.default_rng(5).uniform(-1, 1, 300) ** 3)        # non-uniform, with duplicates
    return np.sort(np.concatenate([r, r[::7], [0.0, 0.5]]))


CASES = [  # id, Q, G, D, grid
    ("q5_d70", 5, 1000, 70, "t21"),
    ("q200_d100_t4096", 200, 1037, 100, "t4096"),
    ("q1000_d36_t1", 1000, 777, 36, "t1"),
    ("q200_d100_nonuniform", 200, 1037, 100, "nonuniform"),
    ("q1000_d52_t21", 1000, 1300, 52, "t21"),
]


@pytest.mark.parametrize("exact", [False, True], ids=["split", "exact_f32"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_all_pairs_equal_slab_counts(case, exact, monkeypatch):
    _, Q, G, D, kind = case
    if exact:
        monkeypatch.setenv("MI355_RANK_EXACT_F32", "1")
    thr = _grid(kind)
    q, g = _randn((Q, D), 11 + Q), _randn((G, D), 12 + G)
    ql, gl = _labels(Q, 7, 13), _labels(G, 7, 14)
    path = EXACT if (exact or D % 4) else SPLIT
    S = M.cosine_scores(q, g)
    assert lib().mi355_rank_last_path() == path
    gen = ql[:, None] == gl[None, :]
    all_ok = torch.ones_like(gen)
    r = M.verification_roc(q, ql, g, gl, thresholds=thr)
    assert lib().mi355_rank_last_path() == path
    _assert_counts(r, _hist_of(S, gen, all_ok, thr))
    # exclude (global rows) with an idx_offset
    off = 1000
    ex = torch.randint(0, G, (Q,), generator=torch.Generator().manual_seed(3)).to(DEV) + off
    ex[::3] = -1
    ok = (torch.arange(G, device=DEV)[None, :] + off) != ex[:, None]
    r = M.verification_roc(q, ql, g, gl, thresholds=thr, exclude=ex, idx_offset=off)
    _assert_counts(r, _hist_of(S, gen, ok, thr))
    # same source: every ordered pair (i, j), i != j
    if Q > 4:
        Ss = M.cosine_scores(q, q)
        r = M.verification_roc(q, ql, thresholds=thr)
        assert lib().mi355_rank_last_path() == path
        _assert_counts(r, _hist_of(Ss, ql[:, None] == ql[None, :], ~torch.eye(Q, dtype=torch.bool, device=DEV), thr))


# ---------------------------------------------------------------- 4. fp16 gallery
@pytest.mark.parametrize("D", [64, 100])
def test_fp16_gallery_counts(D):
    Q, G = 150, 1000
    q, x = _randn((Q, D), 21), _randn((G, D), 22)
    ql, gl = _labels(Q, 5, 23), _labels(G, 5, 24)
    gal = M.Gallery(D, DEV, dtype=torch.float16).add(x, gl)
    v, i = gal.search(q, G)
    assert lib().mi355_rank_last_path() & 0xff == F16_GEMM
    S = torch.empty((Q, G), device=DEV).scatter_(1, i, v)
    ex = torch.randint(0, G, (Q,), generator=torch.Generator().manual_seed(25)).to(DEV)
    ex[::2] = -1
    ok = torch.arange(G, device=DEV)[None, :] != ex[:, None]
    for thr in (GRID, np.linspace(-0.5, 0.5, 4096)):
        r = gal.verification_roc(q, ql, thresholds=thr, exclude=ex)
        assert lib().mi355_rank_last_path() == F16_GEMM
        _assert_counts(r, _hist_of(S, ql[:, None] == gl[None, :], ok, thr))


def test_fp32_gallery_matches_its_search_bits():
    Q, G, D = 40, 900, 64
    q, x = _randn((Q, D), 31), _randn((G, D), 32)
    ql, gl = _labels(Q, 5, 33), _labels(G, 5, 34)
    gal = M.Gallery(D, DEV).add(x, gl)
    S = M.cosine_scores(q, gal.data, gallery_is_normalized=True)
    thr = np.linspace(-0.4, 0.4, 999)
    r = gal.verification_roc(q, ql, thresholds=thr)
    _assert_counts(r, _hist_of(S, ql[:, None] == gl[None, :], torch.ones((Q, G), dtype=torch.bool, device=DEV), thr))


# ---------------------------------------------------------------- 5. scale
def test_same_source_100k_against_blockwise_slab():
    n, D = 100000, 1536
    x = M.synth_fill(n * D, 41, 1, DEV).view(n, D)
    lab = torch.arange(n, device=DEV) % 1000
    thr = np.linspace(-0.1, 0.1, 4096)
    r = M.verification_roc(x, lab, thresholds=thr)
    h = torch.zeros((2, len(thr) + 1), dtype=torch.int64, device=DEV)
    t = torch.as_tensor(thr, device=DEV)
    for q0 in range(0, n, 4096):
        q1 = min(n, q0 + 4096)
        S = M.cosine_scores(x[q0:q1], x)
        b = torch.searchsorted(t, S.double(), right=True)
        gen = lab[q0:q1, None] == lab[None, :]
        rows = torch.arange(q0, q1, device=DEV)
        ok = torch.ones_like(gen)
        ok[rows - q0, rows] = False
        h[0] += torch.bincount(b[ok & gen], minlength=len(thr) + 1)
        h[1] += torch.bincount(b[ok & ~gen], minlength=len(thr) + 1)
        del S, b, gen, ok
    assert int(r["num_genuine"]) == 100 * 99 * 1000 and int(r["num_impostor"]) == n * (n - 1) - 100 * 99 * 1000
    _assert_counts(r, h)


def test_against_float64_within_threshold_noise():
    Q, G, D = 300, 5000, 256
    q, g = _randn((Q, D), 51), _randn((G, D), 52)
    ql, gl = _labels(Q, 3, 53), _labels(G, 3, 54)
    thr = np.linspace(-0.2, 0.2, 41)
    r = M.verification_roc(q, ql, g, gl, thresholds=thr)
    qd, gd = q.double().cpu(), g.double().cpu()
    S = (qd / qd.norm(dim=1, keepdim=True)) @ (gd / gd.norm(dim=1, keepdim=True)).T
    gen = (ql[:, None] == gl[None, :]).cpu()
    for i, t in enumerate(thr):
        near = (S - t).abs() < 1e-5
        want_tp, want_fp = int(((S >= t) & gen).sum()), int(((S >= t) & ~gen).sum())
        assert abs(int(r["tp"][i]) - want_tp) <= int((near & gen).sum()), t
        assert abs(int(r["fp"][i]) - want_fp) <= int((near & ~gen).sum()), t


# ---------------------------------------------------------------- 6. edge cases
def test_few_queries_run_on_the_tiles():
    G, D = 500, 64
    q, g = _randn((8, D), 61), _randn((G, D), 62)
    ql, gl = _labels(8, 3, 63), _labels(G, 3, 64)
    S = M.cosine_scores(q, g)                         # Q = 8: the tiled GEMM (Q <= 4 would take the GEMV)
    thr = np.linspace(-0.5, 0.5, 1001)
    for Q in (1, 3, 4):
        r = M.verification_roc(q[:Q].contiguous(), ql[:Q], g, gl, thresholds=thr)
        assert lib().mi355_rank_last_path() == SPLIT
        _assert_counts(r, _hist_of(S[:Q], ql[:Q, None] == gl[None, :], torch.ones((Q, G), dtype=torch.bool, device=DEV), thr))


def test_nan_rows_count_but_are_never_above_a_threshold():
    Q, G, D = 20, 300, 32
    q, g = _randn((Q, D), 71), _randn((G, D), 72)
    q[3] = float("nan")
    g[17] = float("nan")
    ql, gl = _labels(Q, 3, 73), _labels(G, 3, 74)
    S = M.cosine_scores(q, g)
    assert bool(S[3].isnan().all()) and bool(S[:, 17].isnan().all())
    thr = np.linspace(-1, 1, 21)
    r = M.verification_roc(q, ql, g, gl, thresholds=thr)
    assert int(r["num_genuine"]) + int(r["num_impostor"]) == Q * G
    _assert_counts(r, _hist_of(S, ql[:, None] == gl[None, :], torch.ones((Q, G), dtype=torch.bool, device=DEV), thr))
    assert int(r["tp"][0]) + int(r["fp"][0]) == Q * G - G - Q + 1       # -1 <= every real score; NaN never


def test_single_class_has_no_impostors():
    q = _randn((30, 16), 81)
    r = M.verification_roc(q, torch.zeros(30, dtype=torch.int64, device=DEV))
    assert int(r["num_impostor"]) == 0 and int(r["num_genuine"]) == 30 * 29
    assert bool(r["fpr"].isnan().all()) and not bool(r["tpr"].isnan().any())
    assert int(r["fp"].sum()) == 0 and int(r["tn"].sum()) == 0


def test_two_runs_are_bitwise_equal():
    q, g = _randn((300, 128), 91), _randn((3000, 128), 92)
    ql, gl = _labels(300, 4, 93), _labels(3000, 4, 94)
    for thr in (None, np.linspace(-0.3, 0.3, 4096)):
        a = M.verification_roc(q, ql, g, gl, thresholds=thr)
        b = M.verification_roc(q, ql, g, gl, thresholds=thr)
        for key in a:
            x, y = a[key], b[key]
            if x.dtype == torch.float64:
                x, y = x.view(torch.int64), y.view(torch.int64)
            assert torch.equal(x, y), key


# ---------------------------------------------------------------- 7. sharded
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _same(a, b):
    for key in ("thresholds", "tp", "fp", "fn", "tn", "tpr", "fpr", "auc", "num_genuine", "num_impostor"):
        x, y = a[key], b[key]
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        if not torch.equal(x, y):
            return False
    return True


def _worker(rank, world, port, bounds, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D, Ql = 96, 40
        G = bounds[-1]
        x, q = _randn((G, D), 101), _randn((world * Ql, D), 102)
        gl, ql = _labels(G, 9, 103), _labels(world * Ql, 9, 104)
        ex = torch.randint(0, G, (world * Ql,), generator=torch.Generator().manual_seed(105)).to(DEV)
        ex[::4] = -1
        mine = slice(rank * Ql, (rank + 1) * Ql)
        ok = True
        for dt in (torch.float32, torch.float16):
            gal = M.ShardedGallery(x[bounds[rank]:bounds[rank + 1]].contiguous(), labels=gl[bounds[rank]:bounds[rank + 1]], dtype=dt)
            one = M.Gallery(D, DEV, dtype=dt).add(x, gl)
            for thr, use_ex in ((None, True), (np.linspace(-0.4, 0.4, 4096), False)):
                r = gal.verification_roc(q[mine].contiguous(), ql[mine].contiguous(), thresholds=thr,
                                         exclude=ex[mine].contiguous() if use_ex else None)
                w = one.verification_roc(q, ql, thresholds=thr, exclude=ex if use_ex else None)
                ok = ok and _same(r, w)
        out[rank] = bool(ok)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("bounds", [[0, 3001, 7000], [0, 100, 4321, 7000]], ids=["world2", "world3"])
def test_sharded_matches_one_gallery(bounds):
    world = len(bounds) - 1
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), bounds, out), nprocs=world, join=True)
    assert dict(out) == {r: True for r in range(world)}
