"""fp16 resident gallery on the GPU: the conversion (bit for bit l2_normalize_rows(x).half()), the search against a float64
reference on the same stored rows (GEMV, fused selection and score slab), order / ties / NaN, agreement with the fp32
gallery, the plumbing, and the sharded search (2 and 3 gloo ranks on one GPU)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import MI355Error

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16 = torch.float16


def _randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("D", [1536, 512, 70, 1])
def test_conversion_is_normalize_then_half_bit_for_bit(D):
    x = _randn((1000, D), D)
    gal = M.Gallery(D, DEV, dtype=F16)
    for a, b in [(0, 1), (1, 300), (300, 301), (301, 1000)]:         # several pieces, buffer grows in between
        gal.add(x[a:b])
    assert len(gal) == 1000 and gal.data.shape == (1000, D) and gal.data.dtype == F16
    assert torch.equal(_bits(gal.data), _bits(M.l2_normalize_rows(x).half()))
    ld = (D + 63) // 64 * 64
    assert gal._buf.shape[1] == ld
    assert not gal._buf[:1000, D:].any()                               # the padding is zero


def _ref_scores(gal, q, eps=1e-6):
    """float64 scores of the normalised queries against the stored fp16 rows: (Q, G)."""
    qn = M.l2_normalize_rows(q, eps).double()
    return qn @ gal.data.double().t()


def _check_topk(v, i, s, k, what):
    """v, i: (Q, k) results; s: (Q, G) float64 reference scores."""
    v, i, s = v.cpu().numpy().astype(np.float64), i.cpu().numpy(), s.cpu().numpy()
    Q, G = s.shape
    kk = min(k + 1, G)
    part = np.argpartition(-s, kk - 1, axis=1)[:, :kk] if kk < G else np.tile(np.arange(G), (Q, 1))
    ps = np.take_along_axis(s, part, 1)
    order = np.lexsort((part, -ps), axis=1)
    ref_i = np.take_along_axis(part, order, 1)
    ref_v = np.take_along_axis(ps, order, 1)
    assert np.abs(v - ref_v[:, :k]).max() <= 1e-5, f"{what}: score error {np.abs(v - ref_v[:, :k]).max()}"
    # every returned index carries its own score
    assert np.abs(np.take_along_axis(s, i, 1) - v).max() <= 1e-5, what
    assert all(len(set(r)) == k for r in i.tolist()), f"{what}: repeated index"
    # indices equal the reference except where the reference's neighbouring scores are within 2e-5
    pad = np.full((Q, 1), -np.inf)
    nb = np.concatenate([pad, ref_v, pad], 1) if kk == k else np.concatenate([pad, ref_v], 1)
    close = (np.abs(nb[:, 1:k + 1] - nb[:, :k]) <= 2e-5) | (np.abs(nb[:, 1:k + 1] - nb[:, 2:k + 2]) <= 2e-5)
    bad = (i != ref_i[:, :k]) & ~close
    assert not bad.any(), f"{what}: {int(bad.sum())} index mismatches outside ties"


# D = 48, 150, 200: one, three and four k-steps of the GEMM (its gallery ring is three deep: re-read, exactly full, first reuse)
_SEARCH_SHAPES = ([(G, D) for G in (1, 127, 1000, 100000) for D in (1536, 70)] +
                  [(G, D) for G in (127, 1000) for D in (48, 150, 200)])


@pytest.mark.parametrize("G,D", _SEARCH_SHAPES, ids=[f"{G}-{D}" for G, D in _SEARCH_SHAPES])
def test_search_against_float64_reference(G, D):
    gal = M.Gallery(D, DEV, dtype=F16).add(_randn((G, D), 11 + G))
    qs = _randn((2000, D), 7)
    for Q in (1, 3, 5, 256, 2000):
        q = qs[:Q]
        s = _ref_scores(gal, q)
        for k in (1, 3, 8, 150, 1024):
            if k > G:
                continue
            if Q == 2000 and G == 100000 and k > 8:
                continue                                               # (an 800 MB score slab; k > 8 is covered at Q = 256)
            # (Q = 2000, G = 100k, k <= 8: the fused selection's query block is 640 queries, so this crosses three boundaries)
            v, i = gal.search(q, k)
            assert v.shape == (Q, k) and i.shape == (Q, k) and i.dtype == torch.int64
            _check_topk(v, i, s, k, f"Q={Q} G={G} D={D} k={k}")


@pytest.mark.parametrize("Q", [1, 64])
def test_duplicates_ascend_and_nan_ranks_like_cosine_topk(Q):
    D, G = 1536, 3000
    x = _randn((G, D), 5)
    for r in (17, 40, 2999):
        x[r] = x[5]
    x[7] = float("nan")
    q = x[5:6].repeat(Q, 1) + 1e-3 * _randn((Q, D), 9)
    q[0] = x[5]
    gal = M.Gallery(D, DEV, dtype=F16).add(x)
    v, i = gal.search(q, 8)
    want_v, want_i = M.cosine_topk(q, x, 8)
    assert torch.isnan(v[:, 0]).all() and (i[:, 0] == 7).all()
    assert torch.equal(i[:, 0], want_i[:, 0])
    assert i[0, 1:5].tolist() == [5, 17, 40, 2999]                     # equal scores: ascending index
    assert torch.equal(v[0, 1:5], v[0, 1:2].expand(4))


def test_agrees_with_the_fp32_gallery():
    Q, G, D, k = 256, 100000, 1536, 8
    x, q = _randn((G, D), 21), _randn((Q, D), 22)
    g32 = M.Gallery(D, DEV).add(x)
    g16 = M.Gallery(D, DEV, dtype=F16).add(x)
    v32, i32 = g32.search(q, k)
    v16, i16 = g16.search(q, k)
    delta = 2.0 ** -11 + 1e-5
    qn = M.l2_normalize_rows(q).double()
    s32_at_16 = (qn[:, None, :] * g32.data[i16].double()).sum(-1)      # fp32 gallery's score of every row fp16 returned
    assert (v16.double() - s32_at_16).abs().max().item() <= delta
    must = v32 > v32[:, k - 1:k] + 2 * delta                           # clearly inside the fp32 top-k
    for r in range(Q):
        assert set(i32[r][must[r]].tolist()) <= set(i16[r].tolist()), r


def test_plumbing():
    D, G = 1536, 20000
    x, q = _randn((G, D), 31), _randn((256, D), 32)
    gal = M.Gallery(D, DEV, capacity=G, dtype=F16).add(x)
    for k in (3, 150):
        v, i = gal.search(q, k)
        vo, io = gal.search(q, k, idx_offset=1000)
        assert torch.equal(vo, v) and torch.equal(io, i + 1000)
        a, b = gal.search(q[:128], k), gal.search(q[128:], k)
        assert torch.equal(torch.cat([a[0], b[0]]), v) and torch.equal(torch.cat([a[1], b[1]]), i)
        v2, i2 = gal.search(q, k)
        assert torch.equal(v2, v) and torch.equal(i2, i)
    e = gal.search(q[:0], 5)
    assert e[0].shape == (0, 5) and e[1].shape == (0, 5)
    with pytest.raises(MI355Error, match="embedding dims differ"):
        gal.search(_randn((4, D + 1), 1), 3)
    with pytest.raises(MI355Error, match="out of range"):
        gal.search(q, G + 1)
    with pytest.raises(MI355Error):
        gal.prepare()
    assert M.Gallery(D, DEV, capacity=G, dtype=F16).nbytes * 2 == M.Gallery(D, DEV, capacity=G).nbytes
    assert M.Gallery(70, DEV, capacity=10, dtype=F16).nbytes == 10 * 128 * 2


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_queries_on_another_device_raise():
    gal = M.Gallery(64, DEV, dtype=F16).add(_randn((100, 64), 1))
    with pytest.raises(MI355Error, match="queries on"):
        gal.search(torch.randn(4, 64, device="cuda:1"), 3)


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
        D, Ql = 1536, 64
        x, q = _randn((bounds[-1], D), 41), _randn((world * Ql, D), 42)
        gal = M.ShardedGallery(x[bounds[rank]:bounds[rank + 1]].contiguous(), dtype=F16)
        one = M.Gallery(D, DEV, dtype=F16).add(x)
        ok = gal.total_rows == bounds[-1] and gal.offset == bounds[rank]
        for k in (3, 8, 150):
            v, i = gal.search(q[rank * Ql:(rank + 1) * Ql].contiguous(), k)
            fv, fi = one.search(q, k)
            ok = ok and torch.equal(v, fv) and torch.equal(i, fi)
        out[rank] = bool(ok)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("bounds", [[0, 3001, 20000], [0, 100, 12345, 20000]], ids=["world2", "world3"])
def test_sharded_fp16_matches_one_gallery(bounds):
    world = len(bounds) - 1
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), bounds, out), nprocs=world, join=True)
    assert dict(out) == {r: True for r in range(world)}
