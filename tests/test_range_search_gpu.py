"""Cosine range search on the GPU: the CSR result is exactly ``nonzero(S >= t)`` of the cosine_scores slab on the same path, with
the slab's bits (asserting the path), at float32 rounding boundaries, under every filter, for fp16 galleries (against their
own top-k search and a float64 reference), through the overflow rerun, on edge cases, in a 100k x 100k self-join with planted
cross-class near-duplicates, and sharded over 2 and 3 gloo ranks on one GPU.  The references live here."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import lib
from imageretrievalresearch_amd import rank as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLIT, EXACT, F16_GEMM = 2, 3, 5


def _randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


def _labels(n, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, classes, (n,), generator=g).to(DEV)


def _tiled_scores(q, g, **kw):
    """The slab of q against g on the tiled GEMM: queries padded to 8 rows (Q <= 4 would take the GEMV, whose bits differ)."""
    Q = q.shape[0]
    if Q > 4:
        return M.cosine_scores(q, g, **kw)
    pad = torch.cat([q, torch.ones((8 - Q, q.shape[1]), device=q.device)])
    return M.cosine_scores(pad, g, **kw)[:Q].contiguous()


def _ref(S, t, ok=None, idx_offset=0):
    """nonzero(S >= t) in float64 (NaN never), row-major: rows ascend within a query."""
    hit = S.double() >= t
    if ok is not None:
        hit &= ok
    qi, gi = hit.nonzero(as_tuple=True)
    offsets = torch.zeros(S.shape[0] + 1, dtype=torch.int64, device=S.device)
    offsets[1:] = hit.sum(1).cumsum(0)
    return offsets, gi + idx_offset, S[qi, gi]


def _assert_same(r, ref, what=""):
    off, idx, sc = ref
    assert r.offsets.dtype == torch.int64 and r.indices.dtype == torch.int64 and r.scores.dtype == torch.float32
    assert torch.equal(r.offsets, off), what
    assert torch.equal(r.indices, idx), what
    assert torch.equal(r.scores.view(torch.int32), sc.contiguous().view(torch.int32)), what


def _quantiles(S, ps):
    flat = S.flatten().double().sort().values
    return [float(flat[min(int(p * flat.numel()), flat.numel() - 1)]) for p in ps]


# ---------------------------------------------------------------- 1. exact set and bits against the slab
@pytest.mark.parametrize("D", [64, 70, 1536])
@pytest.mark.parametrize("G", [1000, 12345])
@pytest.mark.parametrize("Q", [1, 3, 4, 5, 130, 257])
def test_equals_slab_nonzero(Q, G, D, monkeypatch):
    q, g = _randn((Q, D), 11 + Q + D), _randn((G, D), 12 + G + D)
    for exact in (False, True):
        if exact:
            monkeypatch.setenv("MI355_RANK_EXACT_F32", "1")
        path = EXACT if (exact or D % 4) else SPLIT
        S = _tiled_scores(q, g)
        for t in _quantiles(S, (0.0, 0.5, 0.99, 0.999, 1.0)) + [-1.0, 0.3, 1.01]:
            r = M.cosine_range(q, g, t)
            assert lib().mi355_rank_last_path() == path, (exact, t)
            _assert_same(r, _ref(S, t), (Q, G, D, exact, t))


# ---------------------------------------------------------------- 2. threshold rounding
def test_threshold_rounding_boundaries():
    Q, G, D = 40, 3000, 96
    q, g = _randn((Q, D), 21), _randn((G, D), 22)
    S = M.cosine_scores(q, g)
    picks = S.flatten()[torch.randperm(Q * G, generator=torch.Generator().manual_seed(23))[:6].to(DEV)].cpu().numpy()
    for s in picks:
        s = np.float32(s)
        up = np.nextafter(s, np.float32(np.inf))
        down = np.nextafter(s, np.float32(-np.inf))
        for t in (float(s),                                         # equal to a score: that pair is in
                  float(np.nextafter(np.float64(s), np.inf)),       # just above it in float64: out
                  float(np.nextafter(np.float64(s), -np.inf)),      # just below it in float64: in
                  (float(s) + float(up)) / 2, (float(s) + float(down)) / 2):   # strictly between two adjacent floats
            assert float(np.float32(t)) != t or t == float(s)          # (every other t lies strictly between floats)
            r = M.cosine_range(q, g, t)
            _assert_same(r, _ref(S, t), t)
        r = M.cosine_range(q, g, float(s))
        qs, gs = (S == torch.tensor(s, device=DEV)).nonzero(as_tuple=True)
        for a, b in zip(qs.tolist(), gs.tolist()):
            seg = r.indices[r.offsets[a]:r.offsets[a + 1]]
            assert b in seg.tolist()
        r = M.cosine_range(q, g, float(np.nextafter(np.float64(s), np.inf)))
        for a, b in zip(qs.tolist(), gs.tolist()):
            assert b not in r.indices[r.offsets[a]:r.offsets[a + 1]].tolist()


# ---------------------------------------------------------------- 3. filters
@pytest.mark.parametrize("D", [64, 70])
def test_filters_equal_masked_slab(D):
    Q, G, off = 150, 2100, 1000
    q, g = _randn((Q, D), 31), _randn((G, D), 32)
    ql, gl = _labels(Q, 4, 33), _labels(G, 4, 34)
    ex = torch.randint(0, G, (Q,), generator=torch.Generator().manual_seed(35)).to(DEV) + off
    ex[::3] = -1
    S = M.cosine_scores(q, g)
    cols = torch.arange(G, device=DEV)[None, :] + off
    t = _quantiles(S, (0.9,))[0]
    same = ql[:, None] == gl[None, :]
    not_ex = cols != ex[:, None]
    for kw, ok in ((dict(label_filter="same"), same), (dict(label_filter="different"), ~same), (dict(exclude=ex), not_ex),
                   (dict(label_filter="different", exclude=ex), ~same & not_ex)):
        r = M.cosine_range(q, g, t, idx_offset=off, query_labels=ql, gallery_labels=gl, **kw)
        _assert_same(r, _ref(S, t, ok, off), kw)
    # exclude compares global rows: a query excluding its own best row loses exactly that row
    q2 = g[:8].clone()
    r = M.cosine_range(q2, g, 0.999, exclude=torch.arange(8, device=DEV))
    assert all(i not in r.indices[r.offsets[i]:r.offsets[i + 1]].tolist() for i in range(8))
    r = M.cosine_range(q2, g, 0.999)
    assert all(i in r.indices[r.offsets[i]:r.offsets[i + 1]].tolist() for i in range(8))


# ---------------------------------------------------------------- 4. fp16 galleries
@pytest.mark.parametrize("D", [64, 100, 1536])
def test_fp16_gallery_against_its_search_and_float64(D):
    Q, G = 37, 1000
    q, x = _randn((Q, D), 41), _randn((G, D), 42)
    gal = M.Gallery(D, DEV, dtype=torch.float16).add(x)
    v, i = gal.search(q, G)                         # every row, descending (the tiled kernel's slab, k > 8)
    rows = gal.data.double()
    qd = q.double()
    S64 = (qd / qd.norm(dim=1, keepdim=True).clamp_min(1e-6)) @ rows.T
    for t in _quantiles(v, (0.5, 0.99, 0.999)):
        r = gal.range_search(q, t)
        assert lib().mi355_rank_last_path() == F16_GEMM
        for a in range(Q):
            keep = v[a].double() >= t
            want_i, order = i[a][keep].sort()
            assert torch.equal(r.indices[r.offsets[a]:r.offsets[a + 1]], want_i), (a, t)
            got = r.scores[r.offsets[a]:r.offsets[a + 1]]
            assert torch.equal(got.view(torch.int32), v[a][keep][order].contiguous().view(torch.int32)), (a, t)
        hit = torch.zeros((Q, G), dtype=torch.bool, device=DEV)
        qi = torch.repeat_interleave(torch.arange(Q, device=DEV), r.offsets[1:] - r.offsets[:-1])
        hit[qi, r.indices] = True
        assert not bool((~hit & (S64 >= t + 1e-5)).any()) and not bool((hit & (S64 <= t - 1e-5)).any())
    # filters on the fp16 gallery: the same entries as the masked full list
    gl = _labels(G, 3, 43)
    ql = _labels(Q, 3, 44)
    gal16 = M.Gallery(D, DEV, dtype=torch.float16).add(x, gl)
    t = _quantiles(v, (0.95,))[0]
    r = gal16.range_search(q, t, query_labels=ql, label_filter="different")
    for a in range(Q):
        keep = (v[a].double() >= t) & (gl[i[a]] != ql[a])
        assert torch.equal(r.indices[r.offsets[a]:r.offsets[a + 1]], i[a][keep].sort().values)


# ---------------------------------------------------------------- 5. overflow and query-block splits
def test_overflow_reruns_once_with_the_same_bits(monkeypatch):
    Q, G, D = 300, 5000, 128
    q, g = _randn((Q, D), 51), _randn((G, D), 52)
    S = M.cosine_scores(q, g)
    t = _quantiles(S, (0.9,))[0]
    want = M.cosine_range(q, g, t)
    _assert_same(want, _ref(S, t))
    monkeypatch.setattr(R, "_cand", R._Workspace())
    monkeypatch.setattr(R, "_MIN_CAPACITY", 7)
    r = M.cosine_range(q, g, t)
    nnz = int(want.offsets[-1])
    assert nnz > 7 and R._cand.get(DEV, 0).numel() == 16 * nnz       # the rerun's buffer: exactly the count it was told
    _assert_same(r, _ref(S, t))
    # the C entry reports the exact count when the candidates are too small, and a call with that capacity fits
    import ctypes as C
    L = lib()
    ws = torch.empty(L.mi355_range_workspace_bytes(Q, G, D), dtype=torch.uint8, device=DEV)
    cand = torch.empty(16 * 10, dtype=torch.uint8, device=DEV)
    n = C.c_int64(-1)
    qc, gc = q.contiguous(), g.contiguous()
    assert L.mi355_cosine_range(qc.data_ptr(), Q, gc.data_ptr(), G, D, 0, 1e-6, t, 0, None, cand.data_ptr(), 10, C.byref(n),
                                ws.data_ptr(), ws.numel(), R.stream_ptr(DEV)) == 0
    assert n.value == nnz
    assert L.mi355_range_compact(cand.data_ptr(), 10, Q, n.value, 0, ws.data_ptr(), ws.numel(), FAKE_OUT(), FAKE_OUT(), FAKE_OUT(),
                                 None) != 0 and b"search again" in L.mi355_last_error()


def FAKE_OUT():
    import ctypes as C
    return C.c_void_p(4096)


def test_query_splits_give_the_same_result():
    Q, G, D = 301, 4000, 64
    q, g = _randn((Q, D), 61), _randn((G, D), 62)
    t = 0.15
    whole = M.cosine_range(q, g, t)
    for cut in (1, 5, 64, 129, 300):
        a, b = M.cosine_range(q[:cut].contiguous(), g, t), M.cosine_range(q[cut:].contiguous(), g, t)
        assert torch.equal(torch.cat([a.offsets, b.offsets[1:] + a.offsets[-1]]), whole.offsets)
        assert torch.equal(torch.cat([a.indices, b.indices]), whole.indices)
        assert torch.equal(torch.cat([a.scores, b.scores]).view(torch.int32), whole.scores.view(torch.int32))


# ---------------------------------------------------------------- 6. edge cases
def test_two_runs_are_bitwise_equal():
    q, g = _randn((257, 1536), 71), _randn((12345, 1536), 72)
    for t in (0.05, 0.1):
        a, b = M.cosine_range(q, g, t), M.cosine_range(q, g, t)
        assert torch.equal(a.offsets, b.offsets) and torch.equal(a.indices, b.indices)
        assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))


def test_duplicates_nan_rows_and_empty_shapes():
    G, D = 1000, 64
    g = _randn((G, D), 81)
    g[17] = g[5]
    g[900] = g[5]
    g[33] = float("nan")
    q = torch.cat([g[5:6], _randn((6, D), 82)])
    q[3] = float("nan")
    r = M.cosine_range(q, g, 0.9999)
    assert r.indices[r.offsets[0]:r.offsets[1]].tolist() == [5, 17, 900]          # every duplicate, ascending
    r = M.cosine_range(q, g, -2.0)
    cnt = (r.offsets[1:] - r.offsets[:-1]).tolist()
    assert cnt == [G - 1, G - 1, G - 1, 0, G - 1, G - 1, G - 1]                      # the NaN row and the NaN query never
    assert 33 not in r.indices.tolist()
    e = M.cosine_range(q[:0], g, 0.5)
    assert e.offsets.tolist() == [0] and e.indices.numel() == 0 and e.scores.numel() == 0
    e = M.cosine_range(q, g[:0], 0.5)
    assert e.offsets.tolist() == [0] * 8 and e.indices.numel() == 0
    with pytest.raises(M.MI355Error, match="max_results"):
        M.cosine_range(q, g, -2.0, max_results=10)
    assert int(M.cosine_range(q, g, -2.0, max_results=6 * (G - 1)).offsets[-1]) == 6 * (G - 1)
    with pytest.raises(M.MI355Error, match="threshold must be finite"):
        M.cosine_range(q, g, float("inf"))


def test_python_checks_with_device_tensors():
    q, g = _randn((6, 32), 91), _randn((50, 32), 92)
    with pytest.raises(M.MI355Error, match="needs query_labels"):
        M.cosine_range(q, g, 0.1, label_filter="same")
    with pytest.raises(M.MI355Error, match="embedding dims differ"):
        M.cosine_range(q, g[:, :16], 0.1)
    with pytest.raises(M.MI355Error, match=r"query_labels must have shape \(6,\)"):
        M.cosine_range(q, g, 0.1, label_filter="same", query_labels=_labels(5, 2, 1), gallery_labels=_labels(50, 2, 2))
    with pytest.raises(M.MI355Error, match="must hold integers"):
        M.cosine_range(q, g, 0.1, exclude=torch.zeros(6, device=DEV))
    with pytest.raises(M.MI355Error, match="must live on the GPU"):
        M.cosine_range(q, g, 0.1, exclude=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(M.MI355Error, match="must live on the GPU"):
        M.cosine_range(q, g.cpu(), 0.1)
    with pytest.raises(M.MI355Error, match="label_filter must be"):
        M.cosine_range(q, g, 0.1, label_filter="all")


def test_prepared_gallery_searches_its_fp32_rows():
    Q, G, D = 20, 3000, 128
    q, x = _randn((Q, D), 95), _randn((G, D), 96)
    plain = M.Gallery(D, DEV).add(x)
    prep = M.Gallery(D, DEV).add(x).prepare()
    S = M.cosine_scores(q, plain.data, gallery_is_normalized=True)
    t = _quantiles(S, (0.99,))[0]
    a, b = plain.range_search(q, t), prep.range_search(q, t)
    _assert_same(a, _ref(S, t))
    _assert_same(b, _ref(S, t))


# ---------------------------------------------------------------- 7. a 100k x 100k self-join with planted near-duplicates
def test_self_join_finds_planted_cross_class_duplicates():
    n, D, t = 100000, 1536, 0.9
    x = M.synth_fill(n * D, 41, 1, DEV).view(n, D)
    lab = torch.arange(n, device=DEV) % 1000
    gen = torch.Generator().manual_seed(7)
    perm = torch.randperm(n, generator=gen)
    a, b, c = perm[:20].to(DEV), perm[20:40].to(DEV), int(perm[40])
    b = torch.where(lab[a] == lab[b], (b + 1) % n, b)                      # different classes
    assert bool((lab[a] != lab[b]).all()) and torch.cat([a, b]).unique().numel() == 40
    x[b] = x[a] + 1e-3 * _randn((20, D), 8)
    c2 = (c + 1000) % n                                                    # a same-class near-duplicate is not reported
    assert c2 not in torch.cat([a, b]).tolist()
    x[c2] = x[c] * 1.0001
    r = M.cosine_range(x, x, t, query_labels=lab, gallery_labels=lab, label_filter="different",
                       exclude=torch.arange(n, device=DEV))
    qi = torch.repeat_interleave(torch.arange(n, device=DEV), r.offsets[1:] - r.offsets[:-1])
    got = sorted(zip(qi.tolist(), r.indices.tolist()))
    want = sorted([(int(i), int(j)) for i, j in zip(a, b)] + [(int(j), int(i)) for i, j in zip(a, b)])
    assert got == want
    # and the blockwise slab under the same mask, bit for bit
    offs, idx, sc = [torch.zeros(1, dtype=torch.int64, device=DEV)], [], []
    for q0 in range(0, n, 4096):
        q1 = min(n, q0 + 4096)
        S = M.cosine_scores(x[q0:q1], x)
        rows = torch.arange(q0, q1, device=DEV)
        ok = lab[q0:q1, None] != lab[None, :]
        ok[rows - q0, rows] = False
        o, i, s = _ref(S, t, ok)
        offs.append(o[1:] + offs[-1][-1])
        idx.append(i)
        sc.append(s)
        del S, ok
    _assert_same(r, (torch.cat(offs), torch.cat(idx), torch.cat(sc)))


# ---------------------------------------------------------------- 8. sharded
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _same(a, b):
    return (torch.equal(a.offsets, b.offsets) and torch.equal(a.indices, b.indices)
            and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)))


def _worker(rank, world, port, bounds, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        D, Ql = 96, 40
        G = bounds[-1]
        x, q = _randn((G, D), 101), _randn((world * Ql, D), 102)
        x[bounds[1] + 1] = x[2]                                            # a cross-shard duplicate
        q[0] = x[2]
        gl, ql = _labels(G, 9, 103), _labels(world * Ql, 9, 104)
        ex = torch.randint(0, G, (world * Ql,), generator=torch.Generator().manual_seed(105)).to(DEV)
        ex[::4] = -1
        mine = slice(rank * Ql, (rank + 1) * Ql)
        ok = True
        for dt in (torch.float32, torch.float16):
            gal = M.ShardedGallery(x[bounds[rank]:bounds[rank + 1]].contiguous(), labels=gl[bounds[rank]:bounds[rank + 1]], dtype=dt)
            one = M.Gallery(D, DEV, dtype=dt).add(x, gl)
            for t, kw, full in ((0.2, {}, {}),
                                (0.1, dict(query_labels=ql[mine].contiguous(), label_filter="different", exclude=ex[mine].contiguous()),
                                 dict(query_labels=ql, label_filter="different", exclude=ex))):
                r = gal.range_search(q[mine].contiguous(), t, **kw)
                w = one.range_search(q, t, **full)
                ok = ok and _same(r, w) and int(w.offsets[-1]) > 0
            r = gal.range_search(q[mine].contiguous(), 0.999)
            ok = ok and r.indices[r.offsets[0]:r.offsets[1]].tolist() == [2, bounds[1] + 1]
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
