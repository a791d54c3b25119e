"""``IVFIndex`` and ``IVFPQIndex`` resolve ``nprobe`` / ``probes`` through one routine (``_lists._ListIndex._probes``): the same
table of bad inputs goes through a fake index of either class - built as test_ivf_args.py and test_ivfpq_args.py build theirs -
and both refuse every entry at the same step with the same text, before the library is reached.  No GPU."""
import re

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import _lists, ivf, ivfpq, pq, rank

ROWS, NLIST, Q = 500, 16, 3


def _fake_ivf():
    ix = ivf.IVFIndex.__new__(ivf.IVFIndex)
    g = M.Gallery.__new__(M.Gallery)
    g.rows, g.dim, g.labels = ROWS, 4, None
    g._buf, g.device, g.dtype, g._prepared, g._prepared_rows, g.eps = torch.zeros(ROWS, 4), torch.device("cpu"), torch.float32, None, 0, 1e-6
    ix.gallery, ix.rows, ix.nlist = g, ROWS, NLIST
    ix._longest = np.arange(NLIST + 1) * 10
    ix.centroids = torch.zeros(NLIST, 4)
    return ix, torch.zeros(Q, 4)


def _fake_ivfpq():
    ix = object.__new__(ivfpq.IVFPQIndex)
    ix.pq = pq.PQGallery(64, "cpu", 8)
    ix.pq._codebooks = torch.zeros(8, 256, 8)                               # as if trained
    ix.pq.rows = ROWS                                                       # as if rows had been added
    ix.nlist, ix.rows = NLIST, ROWS
    ix._longest = np.arange(NLIST + 1) * 10
    ix.centroids = torch.zeros(NLIST, 64)
    return ix, torch.zeros(Q, 64)


def _i64(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


# (nprobe, probes, the text both must raise); in the order of the steps: exactly one, 2-D probes, the count, the queries
HOST = [
    (None, None, "give exactly one of nprobe and probes"),
    (2, _i64(Q, 2), "give exactly one of nprobe and probes"),
    (None, _i64(2 * Q), r"probes must be a \(Q, nprobe\) tensor"),
    (None, _i64(Q, 2, 1), r"probes must be a \(Q, nprobe\) tensor"),
    (None, [[0, 1]] * Q, r"probes must be a \(Q, nprobe\) tensor"),
    (0, None, r"nprobe=0 outside \[1, 16\] \(min\(nlist, 1024\)\)"),
    (-1, None, r"nprobe=-1 outside \[1, 16\]"),
    (17, None, r"nprobe=17 outside \[1, 16\]"),
    (1.5, None, r"nprobe=1.5 outside \[1, 16\]"),
    (True, None, r"nprobe=True outside \[1, 16\]"),
    ("2", None, r"nprobe='2' outside \[1, 16\]"),
    (None, _i64(Q, 17), r"nprobe=17 outside \[1, 16\]"),
    (None, _i64(Q, 0), r"nprobe=0 outside \[1, 16\]"),
    (None, _i64(Q + 1, 17), r"nprobe=17 outside \[1, 16\]"),                # the count comes before the rows of probes
    (2, None, "queries must live on the GPU"),                              # host queries: after every count check
    (None, _i64(Q, 2), "queries must live on the GPU"),
]
# with the tensors taken for device tensors: what is checked once the queries are known
PRETEND = [
    (None, _i64(Q + 1, 2), r"probes must be a \(Q=3, nprobe\) tensor, got \(4, 2\)"),
    (None, _i64(0, 2), r"probes must be a \(Q=3, nprobe\) tensor, got \(0, 2\)"),
    (None, torch.zeros(Q, 2), r"probes must hold integers, got torch.float32"),
    (None, torch.zeros(Q, 2, dtype=torch.bool), r"probes must hold integers, got torch.bool"),
]


def _raised(ix, q, nprobe, probes):
    with pytest.raises(M.MI355Error) as e:
        ix.search(q, 3, nprobe, probes=probes)
    return str(e.value)


def _both_refuse(table):
    for nprobe, probes, text in table:
        said = [_raised(*make(), nprobe, probes) for make in (_fake_ivf, _fake_ivfpq)]
        assert said[0] == said[1], (nprobe, probes, said)
        assert re.search(text, said[0]), (text, said[0])


def test_one_routine_serves_both_classes():
    assert ivf.IVFIndex._probes is ivfpq.IVFPQIndex._probes is _lists._ListIndex._probes
    for name in ("_set_lists", "_check_nprobe", "probe", "_fresh", "stale", "nbytes"):
        assert getattr(ivf.IVFIndex, name) is getattr(ivfpq.IVFPQIndex, name) is getattr(_lists._ListIndex, name), name
    assert _lists.MAX_K == 1024


def test_bad_nprobe_and_probes_are_refused_alike(monkeypatch):
    monkeypatch.setattr(ivf, "lib", lambda: pytest.fail("reached the library"))
    monkeypatch.setattr(ivfpq, "lib", lambda: pytest.fail("reached the library"))
    _both_refuse(HOST)
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)
    _both_refuse(PRETEND)
