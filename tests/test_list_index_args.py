"""The four list indexes search through one routine (``_lists._ListIndex._search_lists``, which resolves ``nprobe`` / ``probes``
in ``_probes``): the same table of bad inputs goes through a fake index of every class - built as test_ivf_args.py,
test_ivfpq_args.py, test_ivf_i8_args.py and test_ivfrpq_args.py build theirs - and all refuse every entry at the same step with
the same text, before the library is reached.  No GPU."""
import re

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import _lists, ivf, ivf_i8, ivfpq, ivfrpq, pq, rank

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


def _fake_ivf_i8():
    ix = object.__new__(ivf_i8.Int8IVFIndex)
    ix.i8 = M.Int8Gallery(64, "cpu")
    ix.i8.rows = ROWS                                                       # as if rows had been added
    ix.nlist, ix.rows = NLIST, ROWS
    ix._longest = np.arange(NLIST + 1) * 10
    ix.centroids = torch.zeros(NLIST, 64)
    return ix, torch.zeros(Q, 64)


def _fake_ivfrpq():
    ix = object.__new__(ivfrpq.ResidualIVFPQIndex)
    ix.pq = object.__new__(ivfrpq._ResidualCodes)
    pq.PQGallery.__init__(ix.pq, 64, "cpu", 8)
    ix.pq._codebooks = torch.zeros(8, 256, 8)                               # as if trained
    ix.pq.rows = ROWS                                                       # as if rows had been added
    ix.nlist, ix.rows = NLIST, ROWS
    ix._longest = np.arange(NLIST + 1) * 10
    ix.centroids = torch.zeros(NLIST, 64)
    return ix, torch.zeros(Q, 64)


FAKES = (_fake_ivf, _fake_ivfpq, _fake_ivf_i8, _fake_ivfrpq)
CLASSES = (ivf.IVFIndex, ivfpq.IVFPQIndex, ivf_i8.Int8IVFIndex, ivfrpq.ResidualIVFPQIndex)


def _i64(*shape):
    return torch.zeros(*shape, dtype=torch.int64)


# (nprobe, probes, the text all must raise); in the order of the steps: exactly one, 2-D probes, the count, the queries
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


def _all_refuse(table):
    for nprobe, probes, text in table:
        said = [_raised(*make(), nprobe, probes) for make in FAKES]
        assert len(set(said)) == 1, (nprobe, probes, said)
        assert re.search(text, said[0]), (text, said[0])


def test_one_routine_serves_both_classes():
    assert ivf.IVFIndex._probes is ivfpq.IVFPQIndex._probes is _lists._ListIndex._probes
    for name in ("_set_lists", "_check_nprobe", "probe", "_fresh", "stale", "nbytes"):
        assert getattr(ivf.IVFIndex, name) is getattr(ivfpq.IVFPQIndex, name) is getattr(_lists._ListIndex, name), name
    assert _lists.MAX_K == 1024


def test_one_routine_serves_the_four_classes():
    base = _lists._ListIndex
    for name in ("_probes", "_set_lists", "_check_nprobe", "probe", "_fresh", "stale", "_search_lists", "_recall_lists"):
        for cls in CLASSES:
            assert getattr(cls, name) is getattr(base, name), (cls.__name__, name)
    for cls in CLASSES[:3]:
        assert cls.nbytes is base.nbytes
    assert "nbytes" in vars(ivfrpq.ResidualIVFPQIndex)                      # the codes and codebooks count into it
    # the query blocks and the slab call of the rows scanned in place; the one call of the code scan; the one add
    for name in ("_top_of_lists", "_scan", "_block", "_queries"):
        assert getattr(ivf.IVFIndex, name) is getattr(ivf_i8.Int8IVFIndex, name) is getattr(ivf._SlabIndex, name), name
    for name in ("_top_of_lists", "_scan"):
        assert getattr(ivfrpq.ResidualIVFPQIndex, name) is getattr(ivfpq.IVFPQIndex, name), name
    assert ivfpq.IVFPQIndex.add is ivf_i8.Int8IVFIndex.add is base._add_to_store
    assert "add" in vars(ivfrpq.ResidualIVFPQIndex) and not hasattr(ivf.IVFIndex, "add")   # its own (assignments=); update()
    assert "search" in vars(ivf.IVFIndex) and "search" in vars(ivfpq.IVFPQIndex) and "search" in vars(ivf_i8.Int8IVFIndex)
    # every C entry is named once, as data
    assert [cls._ENTRIES[1] for cls in CLASSES] == ["mi355_ivf_scan", "mi355_ivfpq_search", "mi355_ivf_scan_i8",
                                                    "mi355_ivfpq_residual_search"]
    assert all(cls._ENTRIES[0] == cls._ENTRIES[1] + "_workspace_bytes" for cls in CLASSES)


def _guard_the_library(monkeypatch):
    for module in (ivf, ivfpq, rank):                                       # where the scans and the rescoring are called
        monkeypatch.setattr(module, "lib", lambda: pytest.fail("reached the library"))


def test_bad_nprobe_and_probes_are_refused_alike(monkeypatch):
    _guard_the_library(monkeypatch)
    _all_refuse(HOST)
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)
    _all_refuse(PRETEND)


def test_a_blocks_filter_is_the_batchs_entered_later(monkeypatch):
    """``rank._filter_from``: the per-query arrays move on by q0 int64, the gallery labels and the mode stay, absent stays absent."""
    monkeypatch.setattr(rank, "require_cuda", lambda t, name: None)
    ql, gl, ex = _i64(9), _i64(ROWS), _i64(9)
    dev = torch.device("cpu")
    assert rank._filter_from(None, 4) is None
    for label_filter, exclude in (("same", ex), ("different", None), (None, ex)):
        whole = rank._rank_filter(9, ROWS, dev, ql, gl if label_filter else None, label_filter, exclude)
        assert rank._filter_from(whole, 0) is whole
        for q0 in (2, 8):
            f, keep = rank._filter_from(whole, q0)
            assert keep is whole[1]                                         # the tensors stay alive with the narrowed filter
            assert f.label_mode == whole[0].label_mode and f.gallery_labels == whole[0].gallery_labels
            assert f.query_labels == (ql.data_ptr() + 8 * q0 if label_filter else None)
            assert f.exclude == (ex.data_ptr() + 8 * q0 if exclude is not None else None)


def test_a_bad_k_is_refused_as_a_gallery_refuses_it(monkeypatch):
    """The k rule of every list index is the row store's: ``IVFIndex.search`` and ``PQGallery.search`` say the same."""
    _guard_the_library(monkeypatch)
    store = _fake_ivfpq()[0].pq
    for k in (0, -1, ROWS + 1, 2.0, True, None, "3"):
        with pytest.raises(M.MI355Error) as e:
            store.search(torch.zeros(Q, 64), k)
        said = [str(e.value)]
        for make in FAKES:
            ix, q = make()
            with pytest.raises(M.MI355Error) as e:
                ix.search(q, k, 2)
            said.append(str(e.value))
        assert len(set(said)) == 1, (k, said)
        assert said[0] == f"selected index k out of range: k={k!r} outside [1, {ROWS}] (min(1024, rows))"
