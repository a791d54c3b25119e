"""Feature-map aggregation without a GPU: the new symbols are declared, bound and exported; every guard of the
mi355_aggregate_* entries (rejected before any HIP call, with a message that names the value) and of the Python API; the
workspace sizer; Swin's refusal; and where the public names live."""
import ctypes
import importlib

import pytest
import torch

import imageretrievalresearch_amd as M
from helpers import header_symbols
from imageretrievalresearch_amd import MI355Error, _lib

AG = importlib.import_module("imageretrievalresearch_amd.aggregate")      # the package attribute `aggregate` is the function
NAMES = ["mi355_aggregate_crow", "mi355_aggregate_regions", "mi355_aggregate_sum", "mi355_aggregate_workspace_bytes"]
BIG = 1 << 40


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_are_declared_bound_and_exported():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in _lib.PROTOTYPES and hasattr(raw, name), name
    assert _lib.lib().mi355_abi_version() == 3


def _regions(fm=1, B=2, C=8, H=7, W=7, regs=((0, 0, 7, 7), (3, 3, 4, 4)), R=None, pool=2, p=3.0, pvec=None, eps_clamp=1e-6,
             normalize=1, ret=0, eps=1e-6, out=1, ws=1, ws_bytes=BIG):
    arr = None if regs is None else (ctypes.c_int32 * (4 * len(regs)))(*[v for r in regs for v in r])
    R = len(regs) if R is None else R
    return _lib.lib().mi355_aggregate_regions(fm, B, C, H, W, arr, R, pool, p, pvec, eps_clamp, normalize, ret, eps, out, ws, ws_bytes,
                                              None)


@pytest.mark.parametrize("kw, msg", [
    (dict(fm=None), b"null"), (dict(regs=None, R=1), b"null"), (dict(out=None), b"null"),
    (dict(B=-1), b"B=-1"), (dict(B=(1 << 22) + 1), b"B=4194305"), (dict(C=0), b"C=0"),
    (dict(H=65), b"H=65"), (dict(H=0), b"H=0"), (dict(W=65), b"W=65"), (dict(W=0), b"W=0"),
    (dict(R=0), b"R=0"), (dict(regs=((0, 0, 1, 1),) * 65), b"R=65"),
    (dict(pool=3), b"pool=3"), (dict(pool=-1), b"pool=-1"),
    (dict(p=0.0), b"p=0"), (dict(p=-1.0), b"p=-1"), (dict(p=64.5), b"p=64.5"), (dict(p=float("nan")), b"p=nan"),
    (dict(eps_clamp=0.0), b"eps_clamp=0"), (dict(eps=-1.0), b"eps=-1"), (dict(eps=float("inf")), b"eps=inf"),
    (dict(regs=((0, 0, 7, 7), (4, 0, 4, 4))), b"region 1 = (y0=4, x0=0, h=4, w=4)"),
    (dict(regs=((0, 4, 7, 4),)), b"region 0"), (dict(regs=((0, 0, 0, 3),)), b"region 0"), (dict(regs=((-1, 0, 2, 2),)), b"y0=-1"),
    (dict(regs=((0, 0, 7, 8),)), b"w=8"), (dict(H=7, W=10, regs=((0, 0, 10, 7),)), b"7x10 map"),
    (dict(ws=None), b"workspace"), (dict(ws_bytes=1024), b"workspace of 1024 bytes"),
])
def test_regions_entry_rejects_bad_arguments(kw, msg):
    assert _regions(**kw) != 0
    assert msg in _err(), (kw, _err())


def test_a_scalar_p_is_not_checked_when_the_pool_does_not_use_it():
    assert _regions(B=0, pool=1, p=0.0, eps_clamp=0.0) == 0
    assert _regions(B=0, pool=2, p=0.0, pvec=1) == 0                # a per-channel tensor replaces the scalar


def _crow(fm=1, B=2, C=8, H=7, W=7, normalize=1, eps=1e-6, out=1, ws=1, ws_bytes=BIG):
    return _lib.lib().mi355_aggregate_crow(fm, B, C, H, W, normalize, eps, out, ws, ws_bytes, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(fm=None), b"null"), (dict(out=None), b"null"), (dict(B=-1), b"B=-1"), (dict(C=0), b"C=0"), (dict(H=65), b"H=65"),
    (dict(W=0), b"W=0"), (dict(eps=float("nan")), b"eps=nan"), (dict(ws=None), b"workspace"), (dict(ws_bytes=16), b"workspace of 16 bytes"),
])
def test_crow_entry_rejects_bad_arguments(kw, msg):
    assert _crow(**kw) != 0
    assert msg in _err(), (kw, _err())


def _sum(vecs=1, B=2, R=3, D=8, normalize=1, eps=1e-6, out=1):
    return _lib.lib().mi355_aggregate_sum(vecs, B, R, D, normalize, eps, out, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(vecs=None), b"null"), (dict(out=None), b"null"), (dict(B=-1), b"B=-1"), (dict(R=0), b"R=0"), (dict(R=65), b"R=65"),
    (dict(D=0), b"D=0"), (dict(eps=-1.0), b"eps=-1"),
])
def test_sum_entry_rejects_bad_arguments(kw, msg):
    assert _sum(**kw) != 0
    assert msg in _err(), (kw, _err())


def test_an_empty_batch_does_nothing_and_needs_no_workspace():
    assert _regions(B=0, ws=None, ws_bytes=0) == 0 and _crow(B=0, ws=None, ws_bytes=0) == 0 and _sum(B=0) == 0


def test_workspace_sizer():
    size = _lib.lib().mi355_aggregate_workspace_bytes
    assert size(0, 1536, 14) == 0
    for bad in ((-1, 8, 1), (1, 0, 1), (1, 8, 0), (1, 8, 65), ((1 << 22) + 1, 8, 1)):
        assert size(*bad) == 0, bad
    one = size(1, 1536, 14)
    assert one >= 2 * 14 * 1536 * 4                                  # the pooled values and a partial sum of squares per channel
    assert size(1, 1536, 1) < one < size(2, 1536, 14) < size(2, 1536, 64)
    assert size(256, 2560, 14) < 1 << 28                             # the largest benchmark shape stays below 256 MiB


def test_python_api_rejects_bad_arguments():
    cpu = torch.zeros(2, 8, 7, 7)
    with pytest.raises(MI355Error, match="GPU"):
        M.aggregate(cpu)
    with pytest.raises(MI355Error, match="tensor"):
        M.aggregate([[1.0]])
    for bad, match in ((lambda: AG._host_regions([(0, 0, 8, 7)], 7, 7), "outside the 7x7 map"),
                       (lambda: AG._host_regions([(0, 0, 7)], 7, 7), r"\(R, 4\)"),
                       (lambda: AG._host_regions([(0.0, 0.0, 1.0, 1.0)], 7, 7), "integer"),
                       (lambda: AG._host_regions([(0, 0, 1, 1)] * 65, 7, 7), "R=65"),
                       (lambda: AG._host_regions(torch.zeros(0, 4, dtype=torch.int64), 7, 7), "R=0"),
                       (lambda: AG._host_regions([(0, 0, 0, 1)], 7, 7), "empty"),
                       (lambda: AG._p_arg(0.0, 8, "cpu"), "p=0.0"), (lambda: AG._p_arg(65, 8, "cpu"), "p=65"),
                       (lambda: AG._p_arg("x", 8, "cpu"), "p must be"), (lambda: AG._p_arg(float("nan"), 8, "cpu"), "p="),
                       (lambda: AG._p_arg(torch.ones(7), 8, "cpu"), r"\(8,\) tensor"),
                       (lambda: AG._p_arg(torch.ones(2, 4), 8, "cpu"), r"\(8,\) tensor"),
                       (lambda: AG._eps(-1.0), "eps"), (lambda: AG._eps("x"), "eps")):
        with pytest.raises(MI355Error, match=match):
            bad()
    assert AG._p_arg(3, 8, "cpu") == (3.0, None) and AG._p_arg(torch.tensor(2.5), 8, "cpu") == (2.5, None)
    pv = AG._p_arg(torch.arange(1, 9), 8, "cpu")[1]
    assert pv.dtype == torch.float32 and pv.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    assert AG._host_regions(((0, 0, 7, 7), (6, 6, 1, 1)), 7, 7).tolist() == [[0, 0, 7, 7], [6, 6, 1, 1]]


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: it reaches the argument checks behind ``require_cuda``; every case below raises
    before the library is called."""
    is_cuda = True


def _fake(*shape):
    return torch.zeros(*shape).as_subclass(_OnGpu)


@pytest.mark.parametrize("shape, kw, match", [
    ((8, 7, 7), {}, "un-pooled"), ((2, 8, 7, 7, 1), {}, "un-pooled"),
    ((2, 8, 7, 7), dict(method="vlad"), "method 'vlad'"), ((2, 8, 7, 7), dict(method=None), "method"),
    ((2, 8, 65, 7), {}, "H=65"), ((2, 8, 7, 0), {}, "W=0"), ((2, 0, 7, 7), {}, "C=0"),
    ((2, 8, 7, 7), dict(p=torch.ones(7)), r"\(8,\) tensor"), ((2, 8, 7, 7), dict(p=0), "p=0"),
    ((2, 8, 7, 7), dict(method="regions"), "needs regions="),
    ((2, 8, 7, 7), dict(method="regions", regions=[(0, 0, 7, 8)]), "outside the 7x7 map"),
    ((2, 8, 7, 7), dict(method="gem", regions=[(0, 0, 7, 7)]), "regions= belongs"),
    ((2, 8, 7, 7), dict(method="crow", regions=[(0, 0, 7, 7)]), "regions= belongs"),
    ((2, 8, 7, 7), dict(method="crow", return_regions=True), "crow"),
    ((2, 8, 7, 7), dict(method="crow", whitening=object()), "crow"),
    ((2, 8, 7, 7), dict(method="gem", pool="max"), "pool= belongs"),
    ((2, 8, 7, 7), dict(method="rmac", pool="median"), "pool 'median'"),
    ((2, 8, 7, 7), dict(method="rmac", whitening=M.Whitening()), "fitted Whitening"),
    ((2, 8, 7, 7), dict(method="rmac", whitening=object()), "fitted Whitening"),
    ((2, 8, 3, 40), dict(method="rmac", levels=4), "R=90"),
    ((2, 8, 7, 7), dict(eps=-1.0), "eps"),
])
def test_aggregate_checks_its_arguments_before_the_library(shape, kw, match):
    with pytest.raises(MI355Error, match=match):
        M.aggregate(_fake(*shape), **kw)


def test_a_whitening_of_another_width_and_regions_with_whitening_are_refused():
    w = M.Whitening.from_moments(10, torch.zeros(6, dtype=torch.float64), torch.eye(6, dtype=torch.float64), 3)
    with pytest.raises(MI355Error, match="dim_in == C = 8"):
        M.aggregate(_fake(2, 8, 7, 7), "rmac", whitening=w)
    w8 = M.Whitening.from_moments(10, torch.zeros(8, dtype=torch.float64), torch.eye(8, dtype=torch.float64), 3)
    with pytest.raises(MI355Error, match="summed descriptor"):
        M.aggregate(_fake(2, 8, 7, 7), "rmac", whitening=w8, return_regions=True)


def test_swin_refuses_and_training_mode_is_refused():
    from imageretrievalresearch_amd.models import MI355Model
    assert "forward_descriptors" not in vars(MI355Model) and callable(MI355Model.forward_descriptors)
    x = torch.zeros(1, 3, 224, 224)
    m = M.create_model("swin_base_patch4_window7_224", num_classes=0).eval()
    with pytest.raises(MI355Error, match="already pooled"):
        m.forward_descriptors(x)
    r = M.create_model("rexnet_100", num_classes=0)
    r.train()
    with pytest.raises(MI355Error, match="forward-only"):
        r.forward_descriptors(x)
    r.eval()
    with pytest.raises(MI355Error, match="GPU"):
        r.forward_descriptors(x)                                     # a CPU input gets as far as forward_features' own check


def test_where_the_public_names_live():
    assert "aggregate" not in M.__all__ and "rmac_regions" not in M.__all__
    assert M.aggregate is AG.aggregate and M.rmac_regions is AG.rmac_regions and callable(M.aggregate)
    from imageretrievalresearch_amd import aggregate, rmac_regions
    assert aggregate is AG.aggregate and rmac_regions is AG.rmac_regions
    assert AG.METHODS == ("spoc", "mac", "gem", "rmac", "crow", "regions")
