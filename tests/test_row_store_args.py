"""The row store behind ``Gallery``, ``Int8Gallery`` and ``PQGallery`` (``rank._RowStore``), the parts that need no GPU: the
growth policy of ``_reserve`` over every buffer of every class, the label append, the recall helper and ``_is_int``."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import pq, rank

DIM = 70                # fp16 and int8 rows are 128 wide: 58 padding columns travel with every row

MAKERS = {
    "fp32": lambda cap: M.Gallery(DIM, "cpu", capacity=cap),
    "fp16": lambda cap: M.Gallery(DIM, "cpu", capacity=cap, dtype=torch.float16),
    "int8": lambda cap: M.Int8Gallery(DIM, "cpu", capacity=cap),
    "pq": lambda cap: pq.PQGallery(72, "cpu", 4, capacity=cap),
}
BUFFERS = {"fp32": ("_buf",), "fp16": ("_buf",), "int8": ("_codes", "_scales"), "pq": ("_codes",)}
WIDTH = {"fp32": {"_buf": (70,)}, "fp16": {"_buf": (128,)}, "int8": {"_codes": (128,), "_scales": ()}, "pq": {"_codes": (4,)}}


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).clone()


@pytest.mark.parametrize("cap", [0, 1, 1000])
@pytest.mark.parametrize("kind", sorted(MAKERS))
def test_reserve_grows_every_buffer_by_one_policy_and_keeps_the_live_rows(kind, cap):
    g = MAKERS[kind](cap)
    assert g._BUFFERS == BUFFERS[kind] and issubclass(type(g), rank._RowStore)
    gen = torch.Generator().manual_seed(cap + 1)
    for name in g._BUFFERS:                                                 # every bit of every row, padding included
        buf = getattr(g, name)
        assert tuple(buf.shape) == (cap,) + WIDTH[kind][name]
        raw = torch.randint(0, 256, (buf.numel() * buf.element_size(),), dtype=torch.uint8, generator=gen)
        buf.view(-1).view(torch.uint8).copy_(raw)
    g.rows = cap                                                            # every row is live
    before = {name: getattr(g, name) for name in g._BUFFERS}
    live = {name: _bytes(t) for name, t in before.items()}
    g._reserve(cap)
    g._reserve(cap - 1)
    assert all(getattr(g, name) is before[name] for name in g._BUFFERS)     # enough room: nothing is reallocated
    g._reserve(cap + 1)
    want_cap = max(cap + 1, int(cap * 1.5) + 1024)
    for name in g._BUFFERS:
        new = getattr(g, name)
        assert new is not before[name] and new.dtype == before[name].dtype and new.device == before[name].device
        assert tuple(new.shape) == (want_cap,) + WIDTH[kind][name], (name, new.shape)
        assert torch.equal(_bytes(new[:cap]), live[name]), name
    assert g.rows == cap and len(g) == cap


def test_reserve_jumps_to_what_is_asked_when_that_is_more():
    g = M.Int8Gallery(DIM, "cpu", capacity=10)
    g._reserve(5000)
    assert g._codes.shape[0] == 5000 and g._scales.shape[0] == 5000
    g._reserve(5001)
    assert g._codes.shape[0] == int(5000 * 1.5) + 1024 == g._scales.shape[0]


@pytest.mark.parametrize("kind", sorted(MAKERS))
def test_labels_are_appended_as_int64_in_order(kind):
    g = MAKERS[kind](0)
    g._add_labels(None)
    assert g.labels is None
    g._add_labels(torch.tensor([5, 3], dtype=torch.int32))                  # None, then labels
    assert g.labels.dtype == torch.int64 and g.labels.tolist() == [5, 3]
    g._add_labels(torch.tensor([9, -1, 5], dtype=torch.int32))              # labels, then labels
    assert g.labels.dtype == torch.int64 and g.labels.tolist() == [5, 3, 9, -1, 5]
    held = g.labels
    g._add_labels(None)                                                     # labels, then None: left as they were
    assert g.labels is held and g.labels.tolist() == [5, 3, 9, -1, 5]


@pytest.mark.parametrize("kind", ["fp32", "fp16", "int8"])
def test_add_checks_its_rows_before_anything_else(kind, monkeypatch):
    g = MAKERS[kind](0)
    how = {"normalized": False} if kind == "int8" else {}
    assert g._append(torch.zeros(0, DIM), torch.tensor([], dtype=torch.int32), **how) is g
    assert g.rows == 0 and g.labels.dtype == torch.int64 and g.labels.numel() == 0      # an empty block needs no GPU
    with pytest.raises(M.MI355Error, match="GPU"):
        g.add(torch.zeros(2, DIM))
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)         # pretend: the shape is refused before any launch
    for bad in (torch.zeros(2, DIM + 1), torch.zeros(DIM), torch.zeros(1, 2, DIM)):
        with pytest.raises(M.MI355Error, match=rf"gallery rows must be \(n,{DIM}\)"):
            g.add(bad)
    assert g.rows == 0


def test_recall_helper_against_a_brute_force_loop():
    got = torch.tensor([[0, 1, 2], [3, 3, 4], [5, 6, 7], [1, 1, 1]])
    want = torch.tensor([[2, 1, 0], [3, 3, 9], [8, 9, 10], [1, 2, 3]])       # repeated indices on either side
    mean, per = rank._recall(got, want, 3)
    brute = [sum(1 for w in want[q].tolist() if w in got[q].tolist()) / 3 for q in range(4)]
    assert brute == [1.0, 2 / 3, 0.0, 1 / 3]
    assert per.dtype == torch.float64 and per.tolist() == brute and mean == float(np.mean(brute))
    none = torch.empty((0, 3), dtype=torch.int64)
    mean, per = rank._recall(none, none, 3)
    assert mean == 1.0 and per.shape == (0,) and per.dtype == torch.float64


def test_is_int():
    assert [rank._is_int(x) for x in (3, np.int64(3), True, 3.0, None, "3")] == [True, True, False, False, False, False]
    assert pq._is_int is rank._is_int
