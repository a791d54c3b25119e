"""Alpha query expansion and DBA on the GPU: the expansion kernel (mi355_expand_rows) against float64 and bit for bit against
the same sum built with torch, QE search as the composition of its two rounds, ranking parity with a float64 pipeline,
batch invariance, Gallery.augmented, retrieval_accuracy(query_expansion=) and the sharded search with the real HIP backend."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import imageretrievalresearch_amd as M
import qe_ref
from helpers import assert_topk_matches
from imageretrievalresearch_amd import MI355Error
from imageretrievalresearch_amd import rank as R
from imageretrievalresearch_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CERT = 5e-5


def tolerance(n):
    """Per-row L2 bound: 4e-6, or (n + 2) * 2^-23 - n + 1 fp32 adds and the two normalisations, each a relative 2^-24 at
    worst, with a factor 2 of headroom - for the larger n (tests/test_query_expansion_args.py checks that every bug it must
    catch moves a row by more than 10x this)."""
    return max(4e-6, (n + 2) * 2.0 ** -23)


def _weights_torch(v, alpha):
    """The kernel's w = v ** alpha for alpha in {0, 1, 3}: 1, v, (v * v) * v."""
    if alpha == 0:
        return torch.ones_like(v)
    if alpha == 1:
        return v.clone()
    return (v * v) * v


def _torch_sum(base_n, rows, vals, idx, alpha):
    """x = base + sum_j w_j * row(i_j), one torch op at a time in rank order (mul rounded, then add), skipped slots skipped."""
    G = rows.shape[0]
    x = base_n.clone()
    used = (vals > 0) & (idx >= 0) & (idx < G)
    w = _weights_torch(vals, alpha)
    for j in range(vals.shape[1]):
        r = rows[idx[:, j].clamp(0, G - 1)]
        x = torch.where(used[:, j:j + 1], x + w[:, j:j + 1] * r, x)
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", [1, 70, 1024, 1536])
@pytest.mark.parametrize("n", [1, 10, 64])
def test_kernel_against_float64_and_torch_bits(dtype, D, n):
    qn_, gn_, vals_, idx_, _ = qe_ref.kernel_case(D, n, seed=7 * D + n)
    q, vals, idx = torch.from_numpy(qn_).to(DEV), torch.from_numpy(vals_).to(DEV), torch.from_numpy(idx_).to(DEV)
    g32 = torch.from_numpy(gn_).to(DEV)
    gal = M.Gallery(D, DEV, dtype=dtype).add(g32)
    rows = gal.data.float()                                    # the stored rows, widened exactly
    nan_row = torch.isnan(rows).any(1)
    assert bool(nan_row[-1]) and not bool(nan_row[:-1].any())
    for alpha in (0.0, 1.0, 3.0):
        out = R._expand_rows(q, True, gal._buf, dtype, gal.rows, D, vals, idx, alpha, gal.eps)
        assert torch.isfinite(out).all(), (D, n, alpha)
        ref = qe_ref.expand(qn_, rows.cpu().numpy(), vals_, idx_, alpha)
        err = np.sqrt(((out.cpu().numpy().astype(np.float64) - ref) ** 2).sum(1))
        assert err.max() <= tolerance(n), (dtype, D, n, alpha, err.max())
        # bit identity with the torch sum, normalised by the library's one row normalisation
        x = _torch_sum(M.l2_normalize_rows(q), rows, vals, idx, alpha)
        assert torch.equal(out, M.l2_normalize_rows(x)), (dtype, D, n, alpha)
        # fp16 output (the DBA form: fp16 base rows as they are): fp16 of l2_normalize_rows(x), zero padding
        if dtype == torch.float16 and alpha == 3.0:
            base = gal._buf[: q.shape[0]]
            dst = torch.full((q.shape[0], gal._ld), float("nan"), dtype=torch.float16, device=DEV)
            R._expand_rows(base, False, gal._buf, dtype, gal.rows, D, vals, idx, alpha, gal.eps, out=dst)
            x16 = _torch_sum(base[:, :D].float(), rows, vals, idx, alpha)
            want = M.Gallery(D, DEV, dtype=torch.float16).add(x16)._buf[: q.shape[0]]
            assert torch.equal(dst.view(torch.int16), want.view(torch.int16)), (D, n)


def test_device_and_shape_errors():
    q = torch.randn(4, 16, device=DEV)
    with pytest.raises(MI355Error):
        M.expand_queries(q, torch.randn(10, 16), 2)           # gallery on the host
    with pytest.raises(MI355Error):
        M.expand_queries(q, torch.randn(10, 8, device=DEV), 2)
    gal = M.Gallery(16, DEV).add(torch.randn(10, 16, device=DEV))
    with pytest.raises(MI355Error):
        gal.search(q.cpu(), 2, qe=(2, 3.0))
    with pytest.raises(MI355Error):
        gal.search(q, 2, qe=(11, 3.0))                          # n > rows
    assert M.expand_queries(q[:0], torch.randn(10, 16, device=DEV), 2).shape == (0, 16)
    assert gal.expand_queries(q[:0], 2).shape == (0, 16)


def _clustered(n, D, classes, seed, spread):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(classes, D, generator=g)
    lab = torch.randint(0, classes, (n,), generator=g)
    return (centers[lab] + spread * torch.randn(n, D, generator=g)).to(DEV), lab.to(DEV)


def _galleries(x, lab):
    D = x.shape[1]
    return {"fp32": M.Gallery(D, DEV).add(x, lab), "prepared": M.Gallery(D, DEV).add(x, lab).prepare(),
            "fp16": M.Gallery(D, DEV, dtype=torch.float16).add(x, lab)}


@pytest.mark.parametrize("kind", ["fp32", "prepared", "fp16"])
def test_qe_search_is_the_composition_of_its_rounds(kind):
    x, lab = _clustered(1500, 96, 30, 1, 1.2)
    q, ql = x[:64], lab[:64]
    gal = _galleries(x, lab)[kind]
    ex = torch.arange(64, dtype=torch.int64, device=DEV)
    for filt in ({}, {"exclude": ex}, {"label_filter": "same", "query_labels": ql}):
        for n, alpha, k in ((5, 3.0, 4), (12, 0.0, 10), (1, 1.0, 8)):
            v, i = gal.search(q, k, qe=(n, alpha), **filt)
            qe = gal.expand_queries(q, n, alpha, **filt)
            v2, i2 = gal.search(qe, k, **filt)
            assert torch.equal(v, v2) and torch.equal(i, i2), (kind, filt.keys(), n)
            if kind != "fp16":
                qe2 = M.expand_queries(q, gal.data, n, alpha, gallery_is_normalized=True, gallery_labels=lab, **filt)
                if kind == "fp32":
                    assert torch.equal(qe, qe2), (filt.keys(), n)
    # qe=None: exactly today's result
    v0, i0 = gal.search(q, 4)
    v1, i1 = gal.search(q, 4, qe=None)
    assert torch.equal(v0, v1) and torch.equal(i0, i1)


def test_ranking_parity_with_float64_pipeline():
    x, lab = _clustered(4000, 128, 40, 2, 1.3)
    g, q = x[:3600], x[3600:]
    n, alpha, k = 5, 3.0, 8
    (v1r, i1r, S1), qe_r, (v2r, i2r, S2) = qe_ref.qe_pipeline(q.cpu().numpy(), g.cpu().numpy(), n, alpha, k)
    gal = M.Gallery(128, DEV).add(g)
    qe = gal.expand_queries(q, n, alpha)
    v, i = gal.search(q, k, qe=(n, alpha))
    cert = (qe_ref.gaps(S1, n) > CERT) & (qe_ref.gaps(S2, k) > CERT)
    assert cert.sum() > 0.5 * len(cert), cert.sum()
    c = np.nonzero(cert)[0]
    err = np.sqrt(((qe.cpu().numpy()[c].astype(np.float64) - qe_r[c]) ** 2).sum(1))
    assert err.max() <= tolerance(n), err.max()
    assert_topk_matches(v.cpu().numpy()[c], i.cpu().numpy()[c], v2r[c], i2r[c], what="qe search")
    _, i_plain = gal.search(q, k)
    assert (i_plain != i).any(1).sum() > 0, "expansion changed no ranking: the test would be vacuous"


def test_invariance_to_batch_position_size_and_runs():
    x, _ = _clustered(2000, 96, 25, 3, 1.2)
    gal = M.Gallery(96, DEV).add(x[:1800])
    pool = x[1800:]
    ref_q = gal.expand_queries(pool[:64], 6, 3.0)
    ref_r = gal.search(pool[:64], 5, qe=(6, 3.0))
    for lo, size in ((5, 8), (0, 37), (2, 100), (5, 200)):
        b = pool[lo: lo + size].contiguous()
        at = 5 - lo
        e = gal.expand_queries(b, 6, 3.0)
        v, i = gal.search(b, 5, qe=(6, 3.0))
        assert torch.equal(e[at], ref_q[5]), (lo, size)
        assert torch.equal(v[at], ref_r[0][5]) and torch.equal(i[at], ref_r[1][5]), (lo, size)
    assert torch.equal(gal.expand_queries(pool[:64], 6, 3.0), ref_q)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_database_side_augmentation(dtype):
    x, lab = _clustered(700, 64, 20, 4, 1.0)
    gal = M.Gallery(64, DEV, dtype=dtype).add(x, lab)
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    before = gal._buf[: gal.rows].clone()
    n, alpha = 4, 3.0
    aug = gal.augmented(n, alpha, block=128)
    assert aug is not gal and aug.dtype == dtype and aug.dim == 64 and aug.rows == gal.rows
    assert torch.equal(aug.labels, gal.labels) and torch.equal(gal._buf[: gal.rows].view(ibits), before.view(ibits))
    assert getattr(aug, "_prepared", None) is None
    # the self-join with each row left out: no row is its own neighbour
    ex = torch.arange(gal.rows, dtype=torch.int64, device=DEV)
    v, i = gal.search(gal.data.float(), n, exclude=ex)
    assert not (i == ex[:, None]).any()
    rows = gal.data.float()
    fp32_out = R._expand_rows(gal._buf[: gal.rows], False, gal._buf, dtype, gal.rows, 64, v, i, alpha, gal.eps)
    if dtype == torch.float32:
        assert torch.equal(aug.data, fp32_out)
        ref = qe_ref.expand(rows.cpu().numpy(), rows.cpu().numpy(), v.cpu().numpy(), i.cpu().numpy(), alpha,
                            normalize_base=False)
        err = np.sqrt(((aug.data.cpu().numpy().astype(np.float64) - ref) ** 2).sum(1))
        assert err.max() <= tolerance(n), err.max()
    else:
        assert torch.equal(aug.data.view(torch.int16), fp32_out.half().view(torch.int16))
        assert not aug._buf[: aug.rows, 64:].any()
    # the augmented gallery searches like any other
    va, ia = aug.search(x[:10], 3)
    assert ia.shape == (10, 3)


@pytest.mark.parametrize("same_source", [True, False])
def test_retrieval_accuracy_with_query_expansion(same_source):
    ks = (1, 2, 4, 8)
    x, lab = _clustered(1200, 64, 30, 5, 1.0)
    if same_source:
        q, ql, g, gl = x, lab, None, None
        args = ()
    else:
        q, ql, g, gl = x[:300], lab[:300], x[300:], lab[300:]
        args = (g, gl)
    base = M.retrieval_accuracy(q, ql, *args, ks=ks)
    none = M.retrieval_accuracy(q, ql, *args, ks=ks, query_expansion=None)
    for key in ("precision_at_1", "r_precision", "map_at_r", "indices"):
        assert torch.equal(base[key], none[key]), key
    got = M.retrieval_accuracy(q, ql, *args, ks=ks, query_expansion=(3, 3.0))
    qn, gn = q.cpu().numpy(), (q if same_source else g).cpu().numpy()
    ex = np.arange(len(qn)) if same_source else None
    Rq = got["R"].cpu().numpy()
    k = got["indices"].shape[1]
    _, _, (_, i2, _) = qe_ref.qe_pipeline(qn, gn, 3, 3.0, k, ex)
    want = qe_ref.retrieval_metrics(i2, ql.cpu().numpy(), (ql if same_source else gl).cpu().numpy(), Rq, ks)
    tol = 1.5 / len(qn)                       # at most one near-tied relevance flip
    assert abs(got["precision_at_1"].item() - want["precision_at_1"]) <= tol
    for K in ks:
        assert abs(got["recall_at_k"][K].item() - want["recall_at_k"][K]) <= tol
    assert abs(got["r_precision"].item() - want["r_precision"]) <= tol
    assert abs(got["map_at_r"].item() - want["map_at_r"]) <= tol
    if same_source:                           # never expanded with its own row
        e = M.expand_queries(q, q, 3, 3.0, exclude=torch.arange(len(qn), device=DEV))
        assert torch.equal(got["indices"], M.cosine_topk(e, q, k, exclude=torch.arange(len(qn), device=DEV))[1])


# ---- sharded: the real HIP backend in 2 and 3 gloo ranks on one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sharded_worker(rank, world, port, bounds, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import imageretrievalresearch_amd as M
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        G, D, Ql = bounds[-1], 72, 6
        full = M.synth_fill(G * D, 11, synth.NORMAL, DEV).view(G, D)
        centers = M.synth_fill(8 * D, 12, synth.NORMAL, DEV).view(8, D)
        full = full * 0.6 + centers[torch.arange(G, device=DEV) % 8]
        allq = M.synth_fill(world * Ql * D, 13, synth.NORMAL, DEV).view(world * Ql, D) * 0.6 + \
            centers[torch.arange(world * Ql, device=DEV) % 8]
        lab = (torch.arange(G, device=DEV) % 5)
        ql = torch.arange(world * Ql, device=DEV) % 5
        lo, hi = bounds[rank], bounds[rank + 1]
        ok = True
        for dtype in (torch.float32, torch.float16):
            sg = M.ShardedGallery(full[lo:hi].contiguous(), labels=lab[lo:hi], dtype=dtype)
            gal = M.Gallery(D, DEV, dtype=dtype).add(full, lab)
            mine = slice(rank * Ql, (rank + 1) * Ql)
            for filt_all, filt_mine in (({}, {}),
                                        ({"exclude": torch.arange(world * Ql, device=DEV) * 7},
                                         {"exclude": (torch.arange(world * Ql, device=DEV) * 7)[mine]}),
                                        ({"label_filter": "same", "query_labels": ql},
                                         {"label_filter": "same", "query_labels": ql[mine]})):
                v, i = sg.search(allq[mine].contiguous(), 4, qe=(6, 3.0), **filt_mine)
                rv, ri = gal.search(allq, 4, qe=(6, 3.0), **filt_all)
                ok = ok and torch.equal(v, rv) and torch.equal(i, ri)
        out[rank] = bool(ok)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world, bounds", [(2, [0, 0, 301]), (3, [0, 97, 97, 260])])
def test_sharded_qe_equals_one_gallery(world, bounds):
    port = _free_port()
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_sharded_worker, args=(world, port, bounds, out), nprocs=world, join=True)
    assert all(out.get(r) for r in range(world)), dict(out)
