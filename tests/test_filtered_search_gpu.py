"""Label-filtered / leave-one-out top-k on the GPU: bit-exact against the eligible entries of the unfiltered search on every
path (asserting the path that ran), against a float64 reference at 100k rows, the edge cases (duplicates, NaN, too few
eligible rows), the Python checks, and the sharded search (2 and 3 gloo ranks on one GPU)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import MI355Error, lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEMV, SPLIT, EXACT, PREP, F16_GEMM, F16_GEMV, FUSED, BITONIC = 1, 2, 3, 4, 5, 6, 0x100, 0x200


def _randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


def _labels(n, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, classes, (n,), generator=g).to(DEV)


def _eligible(Q, G, ql, gl, mode, exclude, off):
    ok = torch.ones((Q, G), dtype=torch.bool, device=DEV)
    if mode == "same":
        ok &= gl[None, :] == ql[:, None]
    elif mode == "different":
        ok &= gl[None, :] != ql[:, None]
    if exclude is not None:
        ok &= (torch.arange(G, device=DEV)[None, :] + off) != exclude[:, None]
    return ok


def _expected(v_all, i_all, ok, k, off):
    """The eligible entries of the unfiltered (Q, G) ranking, in order, padded with (-inf, -1)."""
    Q = v_all.shape[0]
    ev = torch.full((Q, k), -float("inf"), device=DEV)
    ei = torch.full((Q, k), -1, dtype=torch.int64, device=DEV)
    keep = torch.gather(ok, 1, i_all - off)
    for q in range(Q):
        vv, ii = v_all[q][keep[q]][:k], i_all[q][keep[q]][:k]
        ev[q, :vv.numel()], ei[q, :ii.numel()] = vv, ii
    return ev, ei


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _modes(Q, G, seed):
    ql, gl = _labels(Q, 4, seed), _labels(G, 4, seed + 1)
    ex = torch.randint(0, G, (Q,), generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    ex[::3] = -1
    return [("same", ql, gl, None), ("different", ql, gl, None), (None, None, None, ex), ("same", ql, gl, ex)]


PATHS = [  # id, Q, G, D, k, exact, gallery dtype, expected path
    ("gemv", 3, 1000, 64, 3, False, "f32", GEMV),
    ("gemv_bitonic", 2, 1000, 64, 20, False, "f32", GEMV | BITONIC),
    ("split_fused", 37, 1000, 64, 5, False, "f32", SPLIT | FUSED),
    ("split_fused_tail_tile", 200, 300, 64, 8, False, "f32", SPLIT | FUSED),
    ("small_k_slab", 2, 700, 16384, 4, False, "f32", SPLIT),
    ("bitonic", 37, 1000, 64, 20, False, "f32", SPLIT | BITONIC),
    ("exact_fused", 37, 1000, 64, 5, True, "f32", EXACT | FUSED),
    ("exact_bitonic", 70, 777, 64, 30, True, "f32", EXACT | BITONIC),
    ("nonvec_fused", 37, 1000, 70, 5, False, "f32", EXACT | FUSED),
    ("nonvec_bitonic", 37, 1000, 70, 12, False, "f32", EXACT | BITONIC),
    ("f16_gemm_fused", 150, 1000, 64, 5, False, "f16", F16_GEMM | FUSED),
    ("f16_gemm_bitonic", 37, 1000, 70, 20, False, "f16", F16_GEMM | BITONIC),
    ("f16_gemv", 3, 1000, 64, 3, False, "f16", F16_GEMV),
]


@pytest.mark.parametrize("case", PATHS, ids=[c[0] for c in PATHS])
def test_bit_exact_against_the_unfiltered_search(case, monkeypatch):
    name, Q, G, D, k, exact, dt, path = case
    if exact:
        monkeypatch.setenv("MI355_RANK_EXACT_F32", "1")          # read per call
    off = 5000
    x, q = _randn((G, D), G + D), _randn((Q, D), Q + D)
    gal = M.Gallery(D, DEV, dtype=torch.float16 if dt == "f16" else torch.float32)
    for mode, ql, gl, ex in _modes(Q, G, G + Q):
        gal = M.Gallery(D, DEV, dtype=gal.dtype).add(x, gl if gl is not None else torch.zeros(G, dtype=torch.int64))
        v_all, i_all = gal.search(q, G, idx_offset=off)
        v, i = gal.search(q, k, idx_offset=off, query_labels=ql, label_filter=mode, exclude=ex)
        torch.cuda.synchronize()
        assert lib().mi355_rank_last_path() == path, (name, hex(lib().mi355_rank_last_path()))
        ok = _eligible(Q, G, ql, gl, mode, ex, off)
        ev, ei = _expected(v_all, i_all, ok, k, off)
        assert torch.equal(i, ei), (name, mode)
        assert _same_bits(v, ev), (name, mode)


def test_eligible_rows_only_in_the_last_partial_tile():
    G, D, Q, k, off = 1000, 64, 40, 8, 7
    x, q = _randn((G, D), 1), _randn((Q, D), 2)
    gl = torch.zeros(G, dtype=torch.int64, device=DEV)
    gl[990:] = 5                                                # the last tile holds rows 896..999
    ql = torch.full((Q,), 5, dtype=torch.int64, device=DEV)
    ex = torch.full((Q,), off + 995, dtype=torch.int64, device=DEV)
    for dt in (torch.float32, torch.float16):
        gal = M.Gallery(D, DEV, dtype=dt).add(x, gl)
        v_all, i_all = gal.search(q, G, idx_offset=off)
        for kk in (k, 20):
            v, i = gal.search(q, kk, idx_offset=off, query_labels=ql, label_filter="same", exclude=ex)
            ev, ei = _expected(v_all, i_all, _eligible(Q, G, ql, gl, "same", ex, off), kk, off)
            assert torch.equal(i, ei) and _same_bits(v, ev), (dt, kk)
            assert (i[:, 9:] == -1).all() and (i[:, :9] >= off + 990).all()


def test_prepared_gallery_declines_filters_with_identical_results():
    G, D, Q, k = 1000, 64, 50, 5
    x, q = _randn((G, D), 3), _randn((Q, D), 4)
    gl, ql = _labels(G, 6, 5), _labels(Q, 6, 6)
    plain = M.Gallery(D, DEV).add(x, gl)
    prep = M.Gallery(D, DEV).add(x, gl).prepare()
    for mode, ex in (("same", None), ("different", torch.arange(Q, device=DEV))):
        a = plain.search(q, k, query_labels=ql, label_filter=mode, exclude=ex)
        b = prep.search(q, k, query_labels=ql, label_filter=mode, exclude=ex)
        assert torch.equal(a[1], b[1]) and _same_bits(a[0], b[0])
    prep.search(q, k)
    torch.cuda.synchronize()
    assert lib().mi355_rank_last_path() == PREP | FUSED           # unfiltered searches still use the planes


def _check_against_f64(v, i, s, ok, k):
    """v, i: (Q, k); s: (Q, G) float64 scores; ok: eligibility.  Scores within 1e-5 of the float64 top-k of the eligible
    rows, every index eligible, distinct and carrying its own score; indices equal except at near-ties (2e-5)."""
    sm = s.masked_fill(~ok, -float("inf"))
    rv1, ri1 = torch.topk(sm, k + 1, dim=1)                     # k + 1: the k-th row may tie with the next one
    rv, ri = rv1[:, :k], ri1[:, :k]
    real = torch.arange(k, device=DEV)[None, :] < ok.sum(1, keepdim=True)      # slots an eligible row can fill
    assert torch.equal(i >= 0, real), "pads where eligible rows exist, or rows where none is eligible"
    assert (v[~real] == -float("inf")).all()
    ic = i.clamp(min=0)
    v64 = v.double()
    assert (v64 - rv)[real].abs().max().item() <= 1e-5
    assert torch.gather(ok, 1, ic)[real].all()
    assert (torch.gather(s, 1, ic) - v64)[real].abs().max().item() <= 1e-5
    assert all(len(set(x for x in r if x >= 0)) == sum(x >= 0 for x in r) for r in i.cpu().tolist())
    pad = torch.full((rv.shape[0], 1), -float("inf"), dtype=torch.float64, device=DEV)
    nb = torch.cat([pad, rv1], 1)
    close = ((nb[:, 1:k + 1] - nb[:, :k]).abs() <= 2e-5) | ((nb[:, 1:k + 1] - nb[:, 2:k + 2]).abs() <= 2e-5)
    assert not ((i != ri) & ~close & real).any()


@pytest.mark.parametrize("classes", [10, 1000])
@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_against_float64_reference_100k(classes, dt):
    G, D = 100000, 1536
    x = _randn((G, D), 21)
    gl = _labels(G, classes, 22)
    gal = M.Gallery(D, DEV, dtype=torch.float16 if dt == "f16" else torch.float32).add(x, gl)
    rows = gal.data.double()
    for Q in (256, 1):
        q = _randn((Q, D), 23 + Q)
        ql = _labels(Q, classes, 24)
        s = M.l2_normalize_rows(q).double() @ rows.t()
        ex = torch.randint(0, G, (Q,), generator=torch.Generator().manual_seed(25)).to(DEV)
        for mode in ("same", "different"):
            ok = _eligible(Q, G, ql, gl, mode, ex, 0)
            for k in (3, 100):
                v, i = gal.search(q, k, query_labels=ql, label_filter=mode, exclude=ex)
                _check_against_f64(v, i, s, ok, k)


def test_duplicates_exclude_only_the_named_row():
    D, Q = 64, 12
    base = _randn((300, D), 31)
    x = base.clone()
    x[100], x[40], x[250] = base[7], base[7], base[7]            # three copies of row 7
    q = x[[7] * Q]
    for dt in (torch.float32, torch.float16):
        gal = M.Gallery(D, DEV, dtype=dt).add(x)
        for k in (3, 12):
            v, i = gal.search(q, k, exclude=torch.full((Q,), 7, device=DEV))
            assert (i[:, :3] == torch.tensor([40, 100, 250], device=DEV)).all(), (dt, k)
            assert (v[:, 0] == v[:, 1]).all() and (v[:, 1] == v[:, 2]).all()
            assert not (i == 7).any()


def test_nan_rows_ineligible_never_appear_eligible_come_first():
    D, G, Q = 64, 500, 9
    x = _randn((G, D), 41)
    x[[5, 300, 499]] = float("nan")
    gl = torch.zeros(G, dtype=torch.int64, device=DEV)
    gl[300] = 1                                                  # only NaN row 300 is in class 1
    q = _randn((Q, D), 42)
    for dt in (torch.float32, torch.float16):
        gal = M.Gallery(D, DEV, dtype=dt).add(x, gl)
        for k in (3, 20):
            v, i = gal.search(q, k, query_labels=torch.zeros(Q, dtype=torch.int64, device=DEV), label_filter="same")
            assert (i[:, :2] == torch.tensor([5, 499], device=DEV)).all() and torch.isnan(v[:, :2]).all()
            assert not (i == 300).any()
            v, i = gal.search(q, k, query_labels=torch.ones(Q, dtype=torch.int64, device=DEV), label_filter="same")
            assert (i[:, 0] == 300).all() and torch.isnan(v[:, 0]).all()
            assert (i[:, 1:] == -1).all() and (v[:, 1:] == -float("inf")).all()


@pytest.mark.parametrize("Q", [3, 40])
def test_zero_and_too_few_eligible_rows_give_pads_and_misses(Q):
    D, G = 64, 400
    x = _randn((G, D), 51)
    gl = torch.arange(G, device=DEV) % 100                       # 4 rows per class
    ql = torch.full((Q,), 7, dtype=torch.int64, device=DEV)
    ql[0] = 1000                                                 # no row at all
    for dt in (torch.float32, torch.float16):
        gal = M.Gallery(D, DEV, dtype=dt).add(x, gl)
        for k in (1, 3, 8, 50):
            v, i = gal.search(_randn((Q, D), 52), k, query_labels=ql, label_filter="same")
            assert (i[0] == -1).all() and (v[0] == -float("inf")).all()
            n = min(k, 4)
            assert (gl[i[1:, :n]] == 7).all() and (i[1:, n:] == -1).all() and (v[1:, n:] == -float("inf")).all()
            counts = M.hit_counts(i, ql, gl)
            assert counts.tolist() == [Q - 1, Q - 1]               # the pad-only query counts as a miss


def test_python_side_errors():
    D, G, Q = 16, 50, 4
    gal = M.Gallery(D, DEV).add(_randn((G, D), 61))
    q = _randn((Q, D), 62)
    with pytest.raises(MI355Error, match="needs gallery labels"):
        gal.search(q, 3, query_labels=torch.zeros(Q, dtype=torch.int64, device=DEV), label_filter="same")
    lab = M.Gallery(D, DEV).add(_randn((G, D), 61), torch.zeros(G, dtype=torch.int64))
    with pytest.raises(MI355Error, match="needs query_labels"):
        lab.search(q, 3, label_filter="different")
    with pytest.raises(MI355Error, match=r"shape \(4,\)"):
        lab.search(q, 3, query_labels=torch.zeros(5, dtype=torch.int64, device=DEV), label_filter="same")
    with pytest.raises(MI355Error, match=r"shape \(50,\)"):
        M.cosine_topk(q, _randn((G, D), 61), 3, query_labels=torch.zeros(Q, dtype=torch.int64, device=DEV),
                      gallery_labels=torch.zeros(G - 1, dtype=torch.int64, device=DEV), label_filter="same")
    with pytest.raises(MI355Error, match=r"shape \(4,\)"):
        lab.search(q, 3, exclude=torch.zeros((Q, 1), dtype=torch.int64, device=DEV))
    with pytest.raises(MI355Error, match="must hold integers"):
        lab.search(q, 3, exclude=torch.zeros(Q, device=DEV))
    with pytest.raises(MI355Error, match="GPU"):
        lab.search(q, 3, exclude=torch.zeros(Q, dtype=torch.int64))
    with pytest.raises(MI355Error, match="label_filter must be"):
        lab.search(q, 3, query_labels=torch.zeros(Q, dtype=torch.int64, device=DEV), label_filter="SAME")
    lab.labels = lab.labels[:10]
    with pytest.raises(MI355Error, match="10 labels for 50 rows"):
        lab.search(q, 3, query_labels=torch.zeros(Q, dtype=torch.int64, device=DEV), label_filter="same")
    if torch.cuda.device_count() > 1:
        with pytest.raises(MI355Error, match="is on cuda:1"):
            M.Gallery(D, DEV).add(_randn((G, D), 61), torch.zeros(G, dtype=torch.int64)).search(
                q, 3, exclude=torch.zeros(Q, dtype=torch.int64, device="cuda:1"))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, bounds, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D, Ql = 256, 48
        G = bounds[-1]
        x, q = _randn((G, D), 71), _randn((world * Ql, D), 72)
        gl = torch.arange(G, device=DEV) % 997                  # some classes smaller than k: pads
        gl[:40] = 5000                                          # class 5000 lives only in shard 0
        ql = _labels(world * Ql, 997, 73)
        ql[::5] = 5000
        ex = torch.randint(0, G, (world * Ql,), generator=torch.Generator().manual_seed(74)).to(DEV)
        ex[::4] = -1
        mine = slice(rank * Ql, (rank + 1) * Ql)
        ok = True
        for dt in (torch.float32, torch.float16):
            gal = M.ShardedGallery(x[bounds[rank]:bounds[rank + 1]].contiguous(), labels=gl[bounds[rank]:bounds[rank + 1]],
                                   dtype=dt)
            one = M.Gallery(D, DEV, dtype=dt).add(x, gl)
            for k in (3, 8, 60):
                for mode, use_ex in (("same", False), ("different", True), (None, True), ("same", True)):
                    e = ex if use_ex else None
                    v, i = gal.search(q[mine].contiguous(), k, query_labels=ql[mine].contiguous(), label_filter=mode,
                                      exclude=e[mine].contiguous() if use_ex else None)
                    fv, fi = one.search(q, k, query_labels=ql, label_filter=mode, exclude=e)
                    ok = ok and torch.equal(i, fi) and _same_bits(v, fv)
            ok = ok and bool((fi == -1).any())                   # the pads were exercised
        out[rank] = bool(ok)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("bounds", [[0, 3001, 20000], [0, 100, 12345, 20000]], ids=["world2", "world3"])
def test_sharded_filtered_matches_one_gallery(bounds):
    world = len(bounds) - 1
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), bounds, out), nprocs=world, join=True)
    assert dict(out) == {r: True for r in range(world)}
