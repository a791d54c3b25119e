"""The row-sweep kernel's slab pipeline (k_sweep_mbconv, csrc/sweep_mbconv.hip): constants staged one slab ahead, no barrier
between slabs, one squeeze fold per workgroup.

What a slab inherits from its predecessor in the same workgroup - the staged expand / depthwise constants, band -1's X
fragments, the E buffer parity, its slot of squeeze partials - exists only when a workgroup walks more than one slab.  So every
case runs twice through mi355_mbconv_front_ex with the sweep kernel forced: sweep_csplit = 1 (one workgroup per image walks all
slabs: every slab but the last has a successor) and sweep_csplit = number of slabs (no workgroup has one).  D and the squeeze sums of the
two runs must be bit-identical, and both must meet the float64 tolerances of tests/mbconv_front_ref.py (data, reference and
tolerances are that module's, unchanged).  B = 3 leaves five of the eight image slots of the XCD-padded grid idle; mid = 16 is a
single slab, 40 three slabs with a ragged last one (mid % 16 == 8), 96 six slabs; the classes are EfficientNet-B3a's five and
RexNet's 28 x 28 instance with three k-steps.  D and pool are pre-filled with NaN and followed by a NaN guard."""
import ctypes

import pytest
import torch

from mbconv_front_ref import ACT_NONE, ACT_SILU, GUARD, KERNELS, Case, Data, cdiv, reference

DEV = "cuda:0"
B = 3
# name -> (map, Cin, k, stride, act_d): the model's own input widths (24 at 112, 32 at 56, 48 at 28: two k-steps), RexNet 75 -> 80
CLASSES = {"3_2_112": (112, 24, 3, 2, ACT_SILU), "3_1_56": (56, 32, 3, 1, ACT_SILU), "5_2_56": (56, 32, 5, 2, ACT_SILU),
           "5_1_28": (28, 48, 5, 1, ACT_SILU), "3_2_28": (28, 48, 3, 2, ACT_SILU), "rex_3_1_28_kst3": (28, 80, 3, 1, ACT_NONE)}
MIDS = (16, 40, 96)
_REF = {}                   # (class, mid) -> (Data, reference): computed once, shared by the runs, never changed


def _case(cls, mid, csplit, pool=True):
    m, cin, k, s, ad = CLASSES[cls]
    return Case("sweep", B, m, m, cin, mid, k, s, act_e=ACT_SILU, act_d=ad, csplit=csplit, pool=pool)


def _ref(cls, mid):
    if (cls, mid) not in _REF:
        c = _case(cls, mid, 1)
        d = Data(c)
        _REF[cls, mid] = (d, reference(c, d)[0])
    return _REF[cls, mid]


def _run(c, d):
    """One call of mi355_mbconv_front_ex -> (path, D [B][Ho][Wo][mid], pool [B][mid] or None, guards)."""
    from imageretrievalresearch_amd._lib import MbconvFrontArgs, check, lib, stream_ptr
    we, be = d.we_packed(c)
    x = d.x.to(torch.bfloat16).to(DEV).contiguous()
    we, wd = we.to(torch.bfloat16).to(DEV), d.wd.to(torch.bfloat16).to(DEV).contiguous()
    be, bd = be.to(DEV), d.bd.to(DEV)
    nD, nP = c.B * c.Ho * c.Wo * c.mid, c.B * c.mid
    D = torch.full((nD + GUARD,), float("nan"), device=DEV, dtype=torch.bfloat16)
    P = torch.full((nP + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    a = MbconvFrontArgs(X=x.data_ptr(), We=we.data_ptr(), be=be.data_ptr(), Wd=wd.data_ptr(), bd=bd.data_ptr(), D=D.data_ptr(),
                        pool=P.data_ptr() if c.pool else None, B=c.B, H=c.H, W=c.W, Cin=c.Cin, mid=c.mid, k=c.k, stride=c.stride,
                        act_e=c.act_e, act_d=c.act_d, kernel=KERNELS["sweep"], band_rows=0, sweep_variant=0, sweep_csplit=c.csplit)
    path, nblk = ctypes.c_int(-1), ctypes.c_int(-1)
    check(lib().mi355_mbconv_front_ex(ctypes.byref(a), ctypes.byref(nblk), ctypes.byref(path), stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert nblk.value == 1
    Dh, Ph = D.cpu(), P.cpu()
    return path.value, Dh[:nD].view(c.B, c.Ho, c.Wo, c.mid), Ph[:nP].view(c.B, c.mid), {"D": Dh[nD:], "pool": Ph[nP:]}


def _check(name, c, d, ref):
    path, D, pool, guards = _run(c, d)
    assert path == c.code, f"{name}: ran path {path:#x}, expected {c.code:#x} = {c.instance}, csplit {c.used_csplit}"
    for k, g in guards.items():
        assert torch.isnan(g).all(), f"{name}: wrote past the end of {k}"
    bad = torch.isnan(D.float()).nonzero()
    assert bad.numel() == 0, f"{name}: D unwritten at (image, y, x, channel) {bad[0].tolist()}"
    want, tol = ref["D"]
    rD = ((D.double() - want).abs() / tol).max().item()
    msg = f"sweep pipeline {name:36s} csplit {c.used_csplit}: worst |err| / tol D {rD:.3f}"
    if c.pool:
        bad = torch.isnan(pool).nonzero()
        assert bad.numel() == 0, f"{name}: pool unwritten at (image, channel) {bad[0].tolist()}"
        want, tol = ref["pool"]
        rP = ((pool.double() / (c.Ho * c.Wo) - want).abs() / tol).max().item()
        msg += f" squeeze {rP:.3f}"
    else:
        assert torch.isnan(pool).all(), f"{name}: pool is NULL, yet something wrote the squeeze buffer"
        rP = 0.0
    print(msg)
    assert rD <= 1.0, f"{name}: D |err| / tol {rD:.3f}"
    assert rP <= 1.0, f"{name}: squeeze |err| / tol {rP:.3f}"
    return D, pool


@pytest.mark.gpu
@pytest.mark.parametrize("mid", MIDS)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_a_slab_does_not_depend_on_its_predecessor(cls, mid):
    d, ref = _ref(cls, mid)
    nslab = cdiv(mid, 16)
    one, each = _case(cls, mid, 1), _case(cls, mid, nslab)
    assert one.sweep["kst"] == (3 if cls.startswith("rex") else cdiv(one.Cin, 32)) and one.sweep["ns"] == 1
    assert one.used_csplit == 1 and each.used_csplit == nslab
    D1, P1 = _check(f"{cls}_m{mid}", one, d, ref)
    Dn, Pn = _check(f"{cls}_m{mid}", each, d, ref)
    assert torch.equal(D1.view(torch.int16), Dn.view(torch.int16)), f"{cls} mid {mid}: D differs between csplit 1 and {nslab}"
    assert torch.equal(P1, Pn), f"{cls} mid {mid}: the squeeze sums differ between csplit 1 and {nslab}"


@pytest.mark.gpu
def test_without_a_squeeze_buffer():
    """pool = NULL: no fold, no final barrier; D as with the buffer, and nothing lands where the buffer would be."""
    cls, mid = "5_1_28", 40
    d, ref = _ref(cls, mid)
    D1, _ = _check(f"{cls}_m{mid}_poolnull", _case(cls, mid, 1, pool=False), d, ref)
    Dn, _ = _check(f"{cls}_m{mid}_poolnull", _case(cls, mid, 3, pool=False), d, ref)
    Dp, _ = _check(f"{cls}_m{mid}", _case(cls, mid, 1), d, ref)
    assert torch.equal(D1.view(torch.int16), Dn.view(torch.int16)) and torch.equal(D1.view(torch.int16), Dp.view(torch.int16))
