"""Verification ROC without a GPU: the new C symbols, every argument check of the new entries (each refused before any HIP
call, with a message), the Python-side checks that need no device tensor, and the sharded count-then-all_reduce plumbing
through an injected CPU backend."""
import ctypes as C
import math

import pytest
import torch

from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib
from imageretrievalresearch_amd import rank as R
from imageretrievalresearch_amd.sharded import ShardedGallery

NEW = ["mi355_roc_pairs_workspace_bytes", "mi355_roc_pairs_hist", "mi355_roc_pairs_f16_workspace_bytes",
       "mi355_roc_pairs_hist_f16", "mi355_roc_scores_hist", "mi355_roc_finalize"]
FAKE = C.c_void_p(4096)          # never dereferenced: every call below fails its argument checks first


def _thr(vals):
    return (C.c_double * len(vals))(*vals)


GOOD = _thr([0.0, 0.5, 1.0])


def test_new_symbols_are_declared_bound_and_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(L, name), name


def _pairs(thr=GOOD, T=3, q=FAKE, g=FAKE, ql=FAKE, gl=FAKE, thr_dev=FAKE, hist=FAKE, Q=8, G=100, dim=64, ws=FAKE, wsb=1 << 40):
    return _lib.lib().mi355_roc_pairs_hist(q, Q, g, G, dim, 0, 1e-6, ql, gl, None, 0, thr, thr_dev, T, hist, ws, wsb, None)


def _pairs16(thr=GOOD, T=3, q=FAKE, g=FAKE, ql=FAKE, gl=FAKE, thr_dev=FAKE, hist=FAKE, Q=8, G=100, dim=64, ws=FAKE, wsb=1 << 40):
    return _lib.lib().mi355_roc_pairs_hist_f16(q, Q, g, G, dim, 1e-6, ql, gl, None, 0, thr, thr_dev, T, hist, ws, wsb, None)


def _scores(thr=GOOD, T=3, q=FAKE, g=FAKE, ql=FAKE, gl=FAKE, thr_dev=FAKE, hist=FAKE, Q=8, G=100, dim=64, ws=FAKE, wsb=0):
    # q: scores, ql: class codes, Q: n (g / gl / G / dim / ws unused)
    return _lib.lib().mi355_roc_scores_hist(q, 0, Q, ql, thr, thr_dev, T, hist, None)


def _threshold_cases():
    nan, inf = float("nan"), float("inf")
    return [
        (dict(thr=None), b"null thresholds"),
        (dict(T=0), b"T=0"),
        (dict(thr=_thr([0.0] * 4097), T=4097), b"T=4097"),
        (dict(T=-1), b"T=-1"),
        (dict(thr=_thr([0.5, 0.4]), T=2), b"ascending"),
        (dict(thr=_thr([0.0, nan, 1.0])), b"not finite"),
        (dict(thr=_thr([0.0, 0.5, inf])), b"not finite"),
        (dict(thr=_thr([-inf, 0.5, 1.0])), b"not finite"),
        (dict(thr_dev=None), b"null thresholds_dev"),
        (dict(hist=None), b"null"),
    ]


@pytest.mark.parametrize("entry", [_pairs, _pairs16, _scores], ids=["pairs", "pairs_f16", "scores"])
def test_threshold_and_pointer_checks(entry):
    L = _lib.lib()
    for kw, msg in _threshold_cases():
        assert entry(**kw) != 0, kw
        assert msg in L.mi355_last_error(), (kw, msg, L.mi355_last_error())


@pytest.mark.parametrize("entry", [_pairs, _pairs16], ids=["pairs", "pairs_f16"])
def test_pair_entry_checks(entry):
    L = _lib.lib()
    cases = [
        (dict(ql=None), b"null query_labels/gallery_labels"),
        (dict(gl=None), b"null query_labels/gallery_labels"),
        (dict(q=None), b"null queries/gallery"),
        (dict(g=None), b"null queries/gallery"),
        (dict(Q=0), b"bad shape"),
        (dict(G=0), b"bad shape"),
        (dict(dim=0), b"bad shape"),
        (dict(G=1 << 31), b"shape too large"),
        (dict(ws=None), b"workspace"),
        (dict(wsb=16), b"workspace"),
    ]
    for kw, msg in cases:
        assert entry(**kw) != 0, kw
        assert msg in L.mi355_last_error(), (kw, msg, L.mi355_last_error())


def test_scores_entry_and_finalize_checks():
    L = _lib.lib()
    assert _scores(q=None) != 0 and b"null scores/actual" in L.mi355_last_error()
    assert _scores(ql=None) != 0 and b"null scores/actual" in L.mi355_last_error()
    assert _scores(Q=-1) != 0 and b"bad length" in L.mi355_last_error()
    assert L.mi355_roc_scores_hist(FAKE, 2, 8, FAKE, GOOD, FAKE, 3, FAKE, None) != 0
    assert b"scores_f64" in L.mi355_last_error()
    assert L.mi355_roc_finalize(None, 3, FAKE, FAKE, FAKE, FAKE, None) != 0 and b"null" in L.mi355_last_error()
    for p in range(4):
        args = [FAKE] * 4
        args[p] = None
        assert L.mi355_roc_finalize(FAKE, 3, *args, None) != 0 and b"null" in L.mi355_last_error()
    for T in (0, 4097):
        assert L.mi355_roc_finalize(FAKE, T, FAKE, FAKE, FAKE, FAKE, None) != 0
        assert f"T={T}".encode() in L.mi355_last_error()


def test_workspace_has_no_pair_term():
    L = _lib.lib()
    # normalised queries + one call's split planes + 1/|row|: linear in Q and G, no Q x G slab
    big = L.mi355_roc_pairs_workspace_bytes(100000, 100000, 1536)
    assert big < 100000 * 1536 * 4 + 256 * 2**20
    assert L.mi355_roc_pairs_f16_workspace_bytes(100000, 100000, 1536) < 100000 * 1536 * 4 + 256 * 2**20
    assert L.mi355_roc_pairs_workspace_bytes(0, 10, 8) == 0 and L.mi355_roc_pairs_f16_workspace_bytes(4, 10, 0) == 0
    assert L.mi355_roc_pairs_workspace_bytes(256, 100000, 1536) < 16 * 2**20


def test_python_threshold_checks():
    host, dev = R._roc_thresholds(None, "cpu")
    assert host.dtype == torch.float64 and host.shape == (21,) and torch.equal(host, dev)
    assert host[7].item() == 0.35 and host[-1].item() == 1.0
    for bad, msg in (([], "1-D sequence"), ([[0.1, 0.2]], "1-D sequence"), ([0.0] * 4097, "1-D sequence"),
                     ([0.2, 0.1], "ascending"), ([0.1, float("nan")], "finite"), ([float("inf")], "finite")):
        with pytest.raises(MI355Error, match=msg):
            R._roc_thresholds(bad, "cpu")
    host, _ = R._roc_thresholds([0.5, 0.5, 0.7], "cpu")          # equal neighbours are allowed
    assert host.tolist() == [0.5, 0.5, 0.7]


def test_python_side_errors_without_a_device():
    cpu = torch.zeros(4)
    with pytest.raises(MI355Error, match="must live on the GPU"):
        R.roc_curve(cpu, torch.ones(4))
    with pytest.raises(MI355Error, match="must live on the GPU"):
        R.verification_roc(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(MI355Error, match="must be a tensor"):
        R.roc_curve([0.1, 0.2], torch.ones(2))
    g = R.Gallery(8, "cpu")
    with pytest.raises(MI355Error, match="needs gallery labels"):
        g.verification_roc(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))


def test_roc_float32_ceilings():
    """The fp32 comparison value of each float64 threshold: the smallest float f with (double)f >= t."""
    import numpy as np
    for t in (0.35, 0.45, 0.65, 0.7, 0.9, 0.95, 0.05, 0.1, 0.5, 1.0, -0.35, 1e-45, -1e-300, 1e300, 3.4028234663852886e38):
        f = np.float32(t)
        if float(f) < t:
            f = np.nextafter(f, np.float32(np.inf))
        assert float(f) >= t and (float(np.nextafter(f, np.float32(-np.inf))) < t)
    # 0.35 rounds DOWN to float32: the float32 nearest 0.35 is below it and must count as below 0.35
    assert float(np.float32(0.35)) < 0.35 and float(np.float32(0.5)) == 0.5


class _CpuOps:
    """An injected CPU backend: the pair histogram in float64 torch, the finalize in Python."""

    @staticmethod
    def normalize(rows):
        return rows / rows.norm(dim=1, keepdim=True).clamp_min(1e-6)

    @staticmethod
    def roc_hist(queries, query_labels, gallery_normalized, gallery_labels, exclude, idx_offset, thr, gallery_f16=None):
        _CpuOps.calls.append((queries.shape[0], idx_offset, exclude is not None))
        host, _ = thr
        s = _CpuOps.normalize(queries.double()) @ gallery_normalized.double().T
        gen = query_labels[:, None] == gallery_labels[None, :]
        ok = torch.ones_like(gen)
        if exclude is not None:
            ok &= (torch.arange(gallery_normalized.shape[0])[None, :] + idx_offset) != exclude[:, None]
        b = (s[..., None] >= host).sum(-1)
        T = host.shape[0]
        return torch.stack([torch.bincount(b[ok & gen], minlength=T + 1), torch.bincount(b[ok & ~gen], minlength=T + 1)])

    @staticmethod
    def roc_finalize(hist, thr):
        tp = hist[0].flip(0).cumsum(0).flip(0)[1:]
        fp = hist[1].flip(0).cumsum(0).flip(0)[1:]
        return {"thresholds": thr[1], "tp": tp, "fp": fp, "num_genuine": hist[0].sum(), "num_impostor": hist[1].sum()}


_CpuOps.calls = []


def test_sharded_roc_counts_locally_with_the_shard_offset():
    g = torch.randn(50, 16, generator=torch.Generator().manual_seed(0))
    lab = torch.arange(50) % 5
    gal = ShardedGallery(g, ops=_CpuOps, labels=lab)
    q = torch.randn(6, 16, generator=torch.Generator().manual_seed(1))
    ql = torch.arange(6) % 5
    _CpuOps.calls.clear()
    r = gal.verification_roc(q, ql, exclude=torch.tensor([0, 1, -1, 3, 4, 49]))
    assert _CpuOps.calls == [(6, 0, True)]
    assert int(r["num_genuine"]) + int(r["num_impostor"]) == 6 * 50 - 5
    # rows 0, 1, 3, 4 share their query's label (genuine), row 49 does not
    assert int(r["num_genuine"]) == sum(int((lab == c).sum()) for c in ql.tolist()) - 4
    assert r["tp"].shape == (21,) and math.isclose(float(r["thresholds"][1]), 0.05)
    with pytest.raises(MI355Error, match="needs the shard labels"):
        ShardedGallery(g, ops=_CpuOps).verification_roc(q, ql)
