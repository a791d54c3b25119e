"""Filtered search and retrieval metrics, without a GPU: the new C symbols, the mi355_rank_filter layout, every argument
check of the new entries (each refused before any HIP call), the Python-side checks that need no device tensor, and the
unfiltered sharded search still calling a 4-argument local_topk."""
import ctypes as C
import os
import re

import pytest
import torch

from helpers import ROOT, header_symbols
from imageretrievalresearch_amd import MI355Error, _lib
from imageretrievalresearch_amd import rank as R
from imageretrievalresearch_amd.sharded import ShardedGallery

NEW = ["mi355_rank_topk_filtered", "mi355_rank_topk_f16_filtered", "mi355_rank_last_path", "mi355_clear_pads",
       "mi355_retrieval_metrics"]
FAKE = C.c_void_p(4096)          # never dereferenced: every call below fails its argument checks first


def test_new_symbols_are_declared_bound_and_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name


def _header_struct(name):
    txt = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", txt, re.S).group(1)
    return [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w\s\*]+?)\s*\b(\w+);", body)]


def test_filter_struct_layout_matches_header():
    fields = _header_struct("mi355_rank_filter")
    assert [n for _, n in fields] == [n for n, _ in _lib.RankFilter._fields_]
    off = 0
    for (ctype, name), (pname, _) in zip(fields, _lib.RankFilter._fields_):
        size = 8 if "*" in ctype else 4                  # LP64: pointers 8, int 4 (natural alignment = size)
        off = (off + size - 1) // size * size
        assert getattr(_lib.RankFilter, pname).offset == off, name
        off += size
    assert C.sizeof(_lib.RankFilter) == (off + 7) // 8 * 8 == 32
    txt = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    for const, val in (("MI355_LABEL_ANY", _lib.LABEL_ANY), ("MI355_LABEL_SAME", _lib.LABEL_SAME),
                       ("MI355_LABEL_DIFFERENT", _lib.LABEL_DIFFERENT)):
        assert re.search(const + r"\s*=\s*" + str(val) + r"\b", txt), const


def _filt(mode=0, ql=None, gl=None, ex=None):
    f = _lib.RankFilter()
    f.label_mode, f.query_labels, f.gallery_labels, f.exclude = mode, ql, gl, ex
    return f


def _fp32(f, k=3, out=FAKE, Q=8, G=100):
    L = _lib.lib()
    return L.mi355_rank_topk_filtered(FAKE, Q, FAKE, G, 64, 1, k, 1e-6, 0, f, out, out, FAKE, 1 << 30, None)


def _fp16(f, k=3, out=FAKE, Q=8, G=100):
    L = _lib.lib()
    return L.mi355_rank_topk_f16_filtered(FAKE, Q, FAKE, G, 64, k, 1e-6, 0, f, out, out, FAKE, 1 << 30, None)


@pytest.mark.parametrize("entry", [_fp32, _fp16], ids=["fp32", "fp16"])
def test_every_c_argument_check(entry):
    L = _lib.lib()
    cases = [
        (lambda: entry(None), b"null filter"),
        (lambda: entry(_filt(mode=3)), b"unknown label_mode 3"),
        (lambda: entry(_filt(mode=-1)), b"unknown label_mode -1"),
        (lambda: entry(_filt(mode=1)), b"needs query_labels"),
        (lambda: entry(_filt(mode=2, ql=FAKE)), b"needs query_labels"),
        (lambda: entry(_filt(mode=1, gl=FAKE)), b"needs query_labels"),
        (lambda: entry(_filt(), out=None), b"null"),
        (lambda: entry(_filt(), k=0), b"k=0"),
        (lambda: entry(_filt(), k=1025, G=5000), b"k=1025"),
        (lambda: entry(_filt(), k=101, G=100), b"k=101"),
    ]
    for call, msg in cases:
        assert call() != 0
        assert msg in L.mi355_last_error(), (msg, L.mi355_last_error())


def test_metrics_and_clear_pads_argument_checks():
    L = _lib.lib()
    assert L.mi355_retrieval_metrics(None, 4, 3, FAKE, FAKE, 10, FAKE, FAKE, None) != 0
    assert b"null" in L.mi355_last_error()
    assert L.mi355_retrieval_metrics(FAKE, 4, 3, FAKE, FAKE, 10, None, FAKE, None) != 0
    assert L.mi355_retrieval_metrics(FAKE, 4, 1025, FAKE, FAKE, 10, FAKE, FAKE, None) != 0
    assert b"k=1025" in L.mi355_last_error()
    assert L.mi355_retrieval_metrics(FAKE, 0, 3, FAKE, FAKE, 10, FAKE, FAKE, None) != 0
    assert L.mi355_clear_pads(None, FAKE, 4, 0, 1, None) != 0
    assert L.mi355_clear_pads(FAKE, FAKE, -1, 0, 1, None) != 0
    assert L.mi355_clear_pads(FAKE, FAKE, 0, 0, 1, None) == 0          # nothing to do, no HIP call


def test_python_filter_checks_that_need_no_device():
    with pytest.raises(MI355Error, match="label_filter must be"):
        R._rank_filter(4, 10, "cuda:0", None, None, "similar", None)
    with pytest.raises(MI355Error, match="needs query_labels and gallery labels"):
        R._rank_filter(4, 10, "cuda:0", None, None, "same", None)
    with pytest.raises(MI355Error, match="needs query_labels and gallery labels"):
        R._rank_filter(4, 10, "cuda:0", torch.zeros(4, dtype=torch.int64), None, "different", None)
    with pytest.raises(MI355Error, match="must live on the GPU"):
        R._rank_filter(4, 10, "cuda:0", None, None, None, torch.zeros(4, dtype=torch.int64))
    assert R._rank_filter(4, 10, "cuda:0", torch.zeros(4), torch.zeros(10), None, None) is None   # labels alone filter nothing


def test_unfiltered_sharded_search_keeps_the_four_argument_local_topk():
    from test_sharded_gloo import OracleOps
    calls = []

    class Recording(OracleOps):
        @staticmethod
        def local_topk(queries, gallery_normalized, k, idx_offset):
            calls.append((k, idx_offset))
            return OracleOps.local_topk(queries, gallery_normalized, k, idx_offset)

    g = torch.randn(50, 16, generator=torch.Generator().manual_seed(0))
    gal = ShardedGallery(g, ops=Recording, labels=torch.arange(50) % 5)
    q = torch.randn(6, 16, generator=torch.Generator().manual_seed(1))
    v, i = gal.search(q, 4)
    assert calls == [(4, 0)] and v.shape == (6, 4) and i.shape == (6, 4)
    with pytest.raises(MI355Error, match="label_filter must be"):
        gal.search(q, 4, label_filter="other")


def test_prepared_search_shares_the_argument_checks_of_cosine_topk(monkeypatch):
    """PreparedGallery.search runs the checks every search entry runs: queries on another device than the planes are refused
    (the planes' pointer is never handed to a kernel of another GPU), and an empty query batch gives empty (0, k) results.
    The object is built without its constructor and the is-it-on-a-GPU check is switched off, so no device is needed; neither
    case reaches a library call."""
    monkeypatch.setattr(R, "require_cuda", lambda t, name: None)
    p = object.__new__(R.PreparedGallery)
    p.rows, p.dim, p.planes = 100, 8, torch.empty(16, dtype=torch.uint8, device="meta")
    with pytest.raises(MI355Error, match="queries on cpu but gallery on meta"):
        p.search(torch.zeros(6, 8), 3)
    with pytest.raises(MI355Error, match="embedding dims differ"):
        p.search(torch.zeros(6, 9, device="meta"), 3)
    p.planes = torch.empty(16, dtype=torch.uint8)
    v, i = p.search(torch.zeros(0, 8), 3)
    assert v.shape == (0, 3) and v.dtype == torch.float32 and i.shape == (0, 3) and i.dtype == torch.int64
    with pytest.raises(MI355Error, match="out of range"):
        p.search(torch.zeros(0, 8), 101)
    with pytest.raises(MI355Error, match="more than 4 queries"):
        p.search(torch.zeros(2, 8), 3)                   # the planes alone cannot serve Q <= 4
