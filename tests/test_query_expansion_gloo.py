"""ShardedGallery.search(qe=) on CPU: 2 and 3 gloo ranks (ragged, one empty shard) drive the expansion's exchange - round 1,
the per-rank slab of owned neighbour rows, the exact int32 all_reduce(SUM), the expansion of each rank's own queries, round
2 - with the compute backend injected (numpy); the result must equal one unsharded pipeline bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from imageretrievalresearch_amd import synth
from imageretrievalresearch_amd.sharded import ShardedGallery
from test_sharded_gloo import OracleOps


def _expand_np(base, rows, vals, idx, alpha, eps=1e-6):
    """fp32 numpy stand-in of mi355_expand_rows (rank order, one rounding per operation)."""
    def norm(x):
        return (x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), np.float32(eps))).astype(np.float32)
    x = norm(base.astype(np.float32))
    G = rows.shape[0]
    for j in range(vals.shape[1]):
        v, l = vals[:, j], idx[:, j]
        used = (v > 0) & (l >= 0) & (l < G)
        w = np.where(used, np.power(np.where(used, v, 1), np.float32(alpha)), 0).astype(np.float32)
        x = np.where(used[:, None], x + w[:, None] * rows[np.clip(l, 0, G - 1)], x).astype(np.float32)
    return norm(x)


class QEOps(OracleOps):
    @staticmethod
    def qe_slab(idx, lo, local_rows):
        i = idx.numpy() - lo
        rows = local_rows.numpy()
        slab = np.zeros(i.shape + (rows.shape[1],), np.float32)
        own = (i >= 0) & (i < rows.shape[0])
        slab[own] = rows[i[own]]
        return torch.from_numpy(slab)

    @staticmethod
    def expand(base, slab, vals, idx, alpha, eps):
        Q, n, D = slab.shape
        return torch.from_numpy(_expand_np(base.numpy(), slab.numpy().reshape(Q * n, D), vals.numpy(), idx.numpy(), alpha, eps))


def _unsharded(allq, full, n, alpha, k):
    g = QEOps.normalize(full)
    v, i = QEOps.local_topk(allq, g, n, 0)
    qe = _expand_np(allq.numpy(), g.numpy(), v.numpy(), i.numpy(), alpha)
    return QEOps.local_topk(torch.from_numpy(qe), g, k, 0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, bounds, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        G, D, Ql = bounds[-1], 24, 5
        full = torch.from_numpy(synth.fill(21, G * D, synth.NORMAL).reshape(G, D))
        allq = torch.from_numpy(synth.fill(22, world * Ql * D, synth.NORMAL).reshape(world * Ql, D))
        lo, hi = bounds[rank], bounds[rank + 1]
        sg = ShardedGallery(full[lo:hi].contiguous(), ops=QEOps)
        v, i = sg.search(allq[rank * Ql:(rank + 1) * Ql].contiguous(), 4, qe=(6, 3.0))
        rv, ri = _unsharded(allq, full, 6, 3.0, 4)
        out[rank] = bool(torch.equal(v, rv) and torch.equal(i, ri))
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world, bounds", [(2, [0, 40, 90]), (3, [0, 33, 33, 70])])
def test_sharded_qe_exchange_equals_unsharded(world, bounds):
    port = _free_port()
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_worker, args=(world, port, bounds, out), nprocs=world, join=True)
    assert all(out.get(r) for r in range(world)), dict(out)


def test_construction_and_plain_search_need_no_expansion_methods():
    full = torch.from_numpy(synth.fill(3, 30 * 8, synth.NORMAL).reshape(30, 8))
    sg = ShardedGallery(full, ops=OracleOps)
    v, i = sg.search(full[:4], 3)
    assert i.shape == (4, 3)
