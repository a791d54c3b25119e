"""ShardedGallery.fit_whitening on CPU: 2 and 3 gloo ranks (ragged, one empty shard) drive the exchange of the fit - local
moments, ONE all-gather of the packed [n, sum, outer] vector, the sum in rank order, from_moments on every rank - with the
compute backend injected (numpy float64 moments); every rank must hold the same bits, those of from_moments of the
rank-ordered sum of the shard moments."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from imageretrievalresearch_amd import Whitening, synth
from imageretrievalresearch_amd.sharded import ShardedGallery
from test_sharded_gloo import OracleOps

_TENSORS = ("mean", "matrix", "bias", "eigenvalues", "explained_variance_ratio")


class MomentOps(OracleOps):
    @staticmethod
    def moments(local_rows, gallery_f16=None):
        x = local_rows.numpy().astype(np.float64)
        return torch.from_numpy(x.sum(0)), torch.from_numpy(x.T @ x)


def _full(G, D):
    return torch.from_numpy(synth.fill(31, G * D, synth.NORMAL).reshape(G, D) + np.float32(0.5))


def _expected(full, bounds, d):
    """from_moments of the shard moments added in rank order (shards normalised by the same backend)."""
    D = full.shape[1]
    total = np.zeros(1 + D + D * D)
    for r in range(len(bounds) - 1):
        part = np.zeros_like(total)
        rows = full[bounds[r]:bounds[r + 1]]
        if rows.shape[0]:
            s, o = MomentOps.moments(MomentOps.normalize(rows.contiguous()))
            part[0], part[1: 1 + D], part[1 + D:] = rows.shape[0], s.numpy(), o.numpy().reshape(-1)
        total = part.copy() if r == 0 else total + part
    return Whitening.from_moments(int(total[0]), total[1: 1 + D].copy(), total[1 + D:].reshape(D, D).copy(), d)


def _same_bits(a, b):
    return all(np.array_equal(getattr(a, k).numpy().view(np.uint8), getattr(b, k).numpy().view(np.uint8)) for k in _TENSORS)


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
        G, D, d = bounds[-1], 24, 9
        full = _full(G, D)
        sg = ShardedGallery(full[bounds[rank]:bounds[rank + 1]].contiguous(), ops=MomentOps)
        w = sg.fit_whitening(d, power=0.5, ridge=1e-5)
        ok = _same_bits(w, _expected(full, bounds, d)) and (w.dim_in, w.dim_out, w.num_rows, w.normalize_input) == (D, d, G, True)
        # every rank holds the same bits: compare with rank 0's matrix through one broadcast
        m0 = w.matrix.clone()
        torch.distributed.broadcast(m0, 0)
        out[rank] = bool(ok and torch.equal(m0.view(torch.int32), w.matrix.view(torch.int32)))
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world, bounds", [(2, [0, 40, 90]), (3, [0, 33, 33, 70])])
def test_sharded_fit_gives_every_rank_the_same_bits(world, bounds):
    port = _free_port()
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_worker, args=(world, port, bounds, out), nprocs=world, join=True)
    assert all(out.get(r) for r in range(world)), dict(out)


def test_one_rank_fit_makes_no_collective_call(monkeypatch):
    assert not torch.distributed.is_initialized()

    def boom(*a, **k):
        raise AssertionError("a one-rank ShardedGallery called a collective")

    for name in ("all_gather_into_tensor", "all_reduce", "all_gather", "broadcast"):
        monkeypatch.setattr(torch.distributed, name, boom)
    full = _full(60, 16)
    sg = ShardedGallery(full, ops=MomentOps)
    w = sg.fit_whitening(5)
    assert _same_bits(w, _expected(full, [0, 60], 5)) and w.num_rows == 60


def test_construction_and_search_need_no_moments_method():
    full = _full(30, 8)
    sg = ShardedGallery(full, ops=OracleOps)
    v, i = sg.search(full[:4], 3)
    assert i.shape == (4, 3)
