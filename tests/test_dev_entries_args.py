"""The developer entries mi355_window_attention, mi355_gemm_bf16_ex, mi355_dwconv_se_ex, mi355_mbconv_front_ex and mi355_mbconv_block_ex
(with mi355_mbconv_block_how), the parts that need no GPU: the C-ABI symbols and every argument check (rejected before any HIP call,
with a message)."""
import ctypes

import pytest

from helpers import header_symbols
from imageretrievalresearch_amd import _lib

NEW = ["mi355_window_attention", "mi355_gemm_bf16_ex", "mi355_dwconv_se_ex", "mi355_mbconv_front_ex", "mi355_mbconv_block_ex",
       "mi355_mbconv_block_how"]
P = 1 << 20          # a 16-byte aligned stand-in pointer: nothing is dereferenced when a check fails


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_declared_bound_and_exported():
    for name in NEW:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib().mi355_abi_version() == 3


@pytest.mark.parametrize("args,msg", [
    ((None, P, P, 1, 56, 128, 4, 0), b"null"),
    ((P, None, P, 1, 56, 128, 4, 0), b"null"),
    ((P, P, None, 1, 56, 128, 4, 0), b"null"),
    ((P, P, P, 0, 56, 128, 4, 0), b"bad shape"),
    ((P, P, P, 1, 50, 128, 4, 0), b"multiple of 7"),
    ((P, P, P, 1, 0, 128, 4, 0), b"bad shape"),
    ((P, P, P, 1, 56, 96, 4, 0), b"32 * heads"),
    ((P, P, P, 1, 56, 128, 0, 0), b"32 * heads"),
    ((P, P, P, 1, 56, 128, 4, 2), b"shift"),
    ((P, P, P, 1, 56, 128, 4, -3), b"shift"),
    ((P, P, P, 1, 7, 1024, 32, 3), b"shift"),              # one window covers the map: no shift
    ((P + 8, P, P, 1, 56, 128, 4, 0), b"aligned"),
])
def test_window_attention_argument_errors(args, msg):
    assert _lib.lib().mi355_window_attention(*args, None) != 0
    assert msg in _err(), _err()


def _ok():
    """A valid operand block (M = 100, N = 64, K = 96) with stand-in pointers."""
    return dict(A=P, lda=96, W=P, ldw=96, bias=P, out=P, ldo=64, M=100, N=64, K=96, act=0)


@pytest.mark.parametrize("change,msg", [
    (dict(A=None), b"null"),
    (dict(W=None), b"null"),
    (dict(bias=None), b"null"),
    (dict(out=None), b"null"),
    (dict(M=0), b"bad shape"),
    (dict(N=0), b"bad shape"),
    (dict(K=-8), b"bad shape"),
    (dict(K=92, lda=96, ldw=96), b"multiples of 8"),
    (dict(lda=88), b"lda >= K"),
    (dict(lda=100), b"multiples of 8"),
    (dict(ldw=80), b"multiple of 32"),
    (dict(ldw=112), b"multiple of 32"),
    (dict(ldo=56), b"ldo"),
    (dict(N=60, ldo=64), b"multiples of 8"),
    (dict(ldo=68), b"multiples of 8"),
    (dict(act=6), b"activation"),
    (dict(act=-1), b"activation"),
    (dict(res=P, ldr=64, res_n=0), b"res_n"),
    (dict(res=P, ldr=64, res_n=72), b"res_n"),
    (dict(res=P, ldr=32, res_n=40), b"ldr"),
    (dict(res=P, ldr=42, res_n=40), b"ldr"),
    (dict(gate=P, gate_ld=88, rows_per_img=49), b"gate_ld"),
    (dict(gate=P, gate_ld=98, rows_per_img=49), b"gate_ld"),
    (dict(gate=P, gate_ld=96, rows_per_img=0), b"rows_per_img"),
    (dict(rows_per_img=-1), b"rows_per_img"),
    (dict(M_sel=-5), b"M_sel"),
    (dict(splitk_ws=P), b"workspace"),
    (dict(splitk_ws_bytes=4096), b"workspace"),
    (dict(ln_stats=P), b"ln_colsum"),
    (dict(ln_colsum=P), b"ln_colsum"),
    (dict(A=P + 4), b"aligned"),
    (dict(gate=P + 8, gate_ld=96, rows_per_img=49), b"aligned"),
])
def test_gemm_ex_argument_errors(change, msg):
    a = _ok()
    a.update(change)
    x = _lib.GemmExArgs(**a)
    path = ctypes.c_int(-1)
    assert _lib.lib().mi355_gemm_bf16_ex(ctypes.byref(x), ctypes.byref(path), None) != 0
    assert msg in _err(), _err()
    assert path.value == 0                                # a rejected call reports no branch


def test_gemm_ex_null_block():
    assert _lib.lib().mi355_gemm_bf16_ex(None, None, None) != 0
    assert b"null" in _err()


def test_ex_args_layout_matches_the_header():
    """ctypes lays the structure out as C does (LP64); pinned so that a field added on one side only is caught."""
    G = _lib.GemmExArgs
    assert ctypes.sizeof(G) == 152
    assert (G.out.offset, G.M_sel.offset, G.ln_colsum.offset) == (80, 112, 144)


def _dw_ok():
    """A valid operand block (B = 3, 14x14, C = 40, 3x3 stride 1, SE rd = 10) with stand-in pointers."""
    return dict(in_=P, w=P, bias=P, out=P, B=3, H=14, W=14, C=40, k=3, stride=1, act=1, choice=0,
                se_w1=P, se_b1=P, se_w2t=P, se_b2=P, rd=10, act1=1, gate=P)


_NO_SE = dict(se_w1=None, se_b1=None, se_w2t=None, se_b2=None, gate=None, rd=0)


@pytest.mark.parametrize("change,msg", [
    (dict(in_=None), b"null"),
    (dict(w=None), b"null"),
    (dict(bias=None), b"null"),
    (dict(out=None), b"null"),
    (dict(B=0), b"bad shape"),
    (dict(H=0), b"bad shape"),
    (dict(W=-1), b"bad shape"),
    (dict(W=20000), b"bad shape"),
    (dict(C=0), b"bad shape"),
    (dict(C=36), b"multiple of 8"),
    (dict(B=4096, H=4096, W=4096, C=64), b"too large"),
    (dict(k=7), b"unsupported k"),
    (dict(k=1), b"unsupported k"),
    (dict(stride=3), b"unsupported k"),
    (dict(act=6), b"activation"),
    (dict(act=-1), b"activation"),
    (dict(choice=4), b"choice"),
    (dict(choice=-1), b"choice"),
    (dict(choice=2, stride=2), b"tiled does not take"),        # the row-band kernel is stride 1 only
    (dict(choice=2, W=12), b"tiled does not take"),            # and W >= 14
    (dict(choice=3, k=5), b"mfma does not take"),              # the matrix-pipe kernel is 3x3 stride 1 ...
    (dict(choice=3, W=13), b"mfma does not take"),             # ... even W ...
    (dict(choice=3, C=56), b"mfma does not take"),             # ... C <= 48
    (dict(choice=3, W=2), b"mfma does not take"),
    (dict(se_w1=None), b"go together"),
    (dict(se_b2=None), b"go together"),
    (dict(gate=None), b"go together"),
    (dict(_NO_SE, gate=P), b"go together"),
    (dict(rd=0), b"rd"),
    (dict(rd=513), b"rd"),
    (dict(C=4104), b"C <="),
    (dict(act1=7), b"SE activation"),
    (dict(in_=P + 8), b"16-byte aligned"),
    (dict(bias=P + 4), b"16-byte aligned"),
    (dict(out=P + 2), b"16-byte aligned"),
    (dict(gate=P + 2), b"4-byte aligned"),
    (dict(squeeze=P + 1), b"4-byte aligned"),
])
def test_dwconv_se_ex_argument_errors(change, msg):
    a = _dw_ok()
    a.update(change)
    x = _lib.DwconvExArgs(**a)
    path = ctypes.c_int(-1)
    assert _lib.lib().mi355_dwconv_se_ex(ctypes.byref(x), ctypes.byref(path), None) != 0
    assert msg in _err(), _err()
    assert path.value == 0                                # a rejected call reports no kernel


def test_dwconv_se_ex_null_block():
    assert _lib.lib().mi355_dwconv_se_ex(None, None, None) != 0
    assert b"null" in _err()


def test_dwconv_ex_args_layout_matches_the_header():
    D = _lib.DwconvExArgs
    assert ctypes.sizeof(D) == 120
    assert (D.B.offset, D.choice.offset, D.se_w1.offset, D.rd.offset, D.gate.offset, D.squeeze.offset) == (32, 60, 64, 96, 104, 112)


def _front_ok():
    """A valid operand block (B = 3, 14x14, 24 -> 144, 3x3 stride 1, SiLU / SiLU, kernel auto = late) with stand-in pointers."""
    return dict(X=P, We=P, be=P, Wd=P, bd=P, D=P, pool=P, B=3, H=14, W=14, Cin=24, mid=144, k=3, stride=1, act_e=1, act_d=1)


_AT56 = dict(H=56, W=56)        # a 3x3 stride-1 56x56 layer: the sweep kernel's class 3_1_56, and a band-kernel shape


@pytest.mark.parametrize("change,msg", [
    (dict(X=None), b"null"),
    (dict(We=None), b"null"),
    (dict(be=None), b"null"),
    (dict(Wd=None), b"null"),
    (dict(bd=None), b"null"),
    (dict(D=None), b"null"),
    (dict(B=0), b"bad shape"),
    (dict(B=65536), b"bad shape"),
    (dict(H=0), b"bad shape"),
    (dict(W=-1), b"bad shape"),
    (dict(W=20000), b"bad shape"),
    (dict(Cin=0), b"bad shape"),
    (dict(mid=0), b"bad shape"),
    (dict(mid=40000), b"bad shape"),
    (dict(Cin=20), b"multiples of 8"),
    (dict(mid=148), b"multiples of 8"),
    (dict(B=4096, H=4096, W=4096, kernel=3), b"too large"),
    (dict(k=7), b"unsupported k"),
    (dict(k=1), b"unsupported k"),
    (dict(stride=3), b"unsupported k"),
    (dict(act_e=6), b"activation"),
    (dict(act_d=-1), b"activation"),
    (dict(kernel=4), b"unknown kernel"),
    (dict(kernel=-1), b"unknown kernel"),
    (dict(band_rows=-1), b"out of range"),
    (dict(sweep_variant=5), b"out of range"),
    (dict(sweep_csplit=-2), b"out of range"),
    (dict(sweep_csplit=4096), b"out of range"),
    (dict(X=P + 8), b"16-byte aligned"),
    (dict(be=P + 4), b"16-byte aligned"),
    (dict(D=P + 2), b"16-byte aligned"),
    (dict(pool=P + 4), b"16-byte aligned"),
    (dict(H=15, W=14, k=5), b"unfused"),                              # auto: 210 pixels and 5x5: the plan fuses no such pair
    (dict(_AT56, Cin=72, mid=432), b"unfused"),                       # auto: three k-steps with SiLU / SiLU
    (dict(kernel=1, H=15, W=14), b"late does not take"),              # the whole-image kernel stops at 208 pixels
    (dict(kernel=1, Cin=512, mid=3072), b"late does not take"),       # ... and at the LDS
    (dict(kernel=2), b"sweep does not take"),                         # the sweep kernel has its map classes
    (dict(_AT56, kernel=2, k=5), b"sweep does not take"),
    (dict(_AT56, kernel=2, Cin=72), b"sweep does not take"),          # three k-steps: only RexNet's 3_2_56 with SiLU / none
    (dict(_AT56, kernel=2, Cin=72, stride=2, act_d=1), b"sweep does not take"),
    (dict(H=28, W=28, kernel=2, Cin=136, act_d=0), b"sweep does not take"),     # five k-steps
    (dict(_AT56, kernel=3, Cin=72), b"band does not take"),           # the band kernel has one or two k-steps
    (dict(kernel=3, H=8, W=136), b"band does not take"),              # ... and maps up to 128 wide
    (dict(_AT56, kernel=3, Cin=32, mid=192, band_rows=10), b"exceeds"),          # nine rows of this layer fit the LDS
    (dict(band_rows=2), b"belongs to the band kernel"),
    (dict(_AT56, kernel=2, band_rows=2), b"belongs to the band kernel"),
    (dict(sweep_variant=1), b"belong to the sweep kernel"),
    (dict(_AT56, kernel=3, sweep_csplit=2), b"belong to the sweep kernel"),
])
def test_mbconv_front_ex_argument_errors(change, msg):
    a = _front_ok()
    a.update(change)
    x = _lib.MbconvFrontArgs(**a)
    path, nblk = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.lib().mi355_mbconv_front_ex(ctypes.byref(x), ctypes.byref(nblk), ctypes.byref(path), None) != 0
    assert msg in _err(), _err()
    assert path.value == 0 and nblk.value == 0            # a rejected call reports no kernel


def test_mbconv_front_ex_null_block():
    assert _lib.lib().mi355_mbconv_front_ex(None, None, None, None) != 0
    assert b"null" in _err()


def test_mbconv_front_args_layout_matches_the_header():
    F = _lib.MbconvFrontArgs
    assert ctypes.sizeof(F) == 112
    assert (F.pool.offset, F.B.offset, F.act_d.offset, F.kernel.offset, F.sweep_csplit.offset) == (48, 56, 88, 92, 104)


def _block_ok():
    """A valid operand block (B = 3, 14x14, 96 -> 576 -> 96, 3x3 stride 1, rd 24, SiLU / SiLU, residual on every column: efficientnet_b3a's
    first whole-block shape) with stand-in pointers."""
    return dict(X=P, We=P, be=P, Wd=P, bd=P, W1=P, b1=P, W2=P, b2=P, Wp=P, bp=P, D=P, Y=P, B=3, H=14, W=14, Cin=96, mid=576, Cout=96, k=3,
                stride=1, rd=24, act_e=1, act_d=1, se_act=1, a_relu6=0, has_res=1, res_n=96, norot=0)


_NO_RES = dict(has_res=0, res_n=0)


@pytest.mark.parametrize("change,msg", [
    *[(dict([(p, None)]), b"null") for p in ("X", "We", "be", "Wd", "bd", "W1", "b1", "W2", "b2", "Wp", "bp", "D", "Y")],
    (dict(B=0), b"bad shape"),
    (dict(B=65536), b"bad shape"),
    (dict(H=0), b"bad shape"),
    (dict(W=-1), b"bad shape"),
    (dict(W=20000), b"bad shape"),
    (dict(Cin=0), b"bad shape"),
    (dict(mid=0), b"bad shape"),
    (dict(mid=40000), b"bad shape"),
    (dict(Cout=0), b"bad shape"),
    (dict(rd=0), b"bad shape"),
    (dict(rd=-3), b"bad shape"),
    (dict(Cin=100), b"multiples of 8"),
    (dict(mid=580), b"multiples of 8"),
    (dict(Cout=100), b"multiples of 8"),
    (dict(k=7), b"unsupported k"),
    (dict(k=1), b"unsupported k"),
    (dict(stride=3), b"unsupported k"),
    (dict(stride=0), b"unsupported k"),
    (dict(act_e=6), b"activation"),
    (dict(act_d=-1), b"activation"),
    (dict(se_act=6), b"SE activation"),
    (dict(se_act=-1), b"SE activation"),
    (dict(a_relu6=2), b"flags"),
    (dict(has_res=-1), b"flags"),
    (dict(_NO_RES, Cin=136, mid=816, Cout=232, k=5, stride=2, rd=34, has_res=1, res_n=136), b"stride 1"),
    (dict(res_n=0), b"res_n"),
    (dict(res_n=100), b"res_n"),
    (dict(res_n=104), b"res_n"),                                       # past min(Cin, Cout)
    (dict(Cout=136, res_n=104), b"res_n"),                             # past Cin
    (dict(res_n=-8), b"res_n"),
    (dict(has_res=0), b"without a residual"),
    (dict(norot=16), b"norot"),
    (dict(norot=-1), b"norot"),
    *[(dict([(p, P + off)]), b"16-byte aligned") for p, off in (("X", 8), ("We", 2), ("be", 4), ("Wd", 8), ("bd", 4), ("W1", 8), ("b1", 4),
                                                                 ("W2", 2), ("b2", 8), ("Wp", 8), ("bp", 4), ("D", 2), ("Y", 8))],
    (dict(H=15), b"unsupported shape"),                                # 210 pixels
    (dict(H=7, W=7), b"unsupported shape"),                            # no 7x7 instance with three k-steps
    (dict(_NO_RES, H=7, W=7, Cin=232, mid=1392, Cout=232, k=5, stride=2, rd=58), b"unsupported shape"),      # no stride 2 on 7x7
    (dict(act_e=0), b"unsupported shape"),                             # the expand activation is SiLU
    (dict(act_d=2), b"unsupported shape"),
    (dict(mid=2568), b"unsupported shape"),
    (dict(rd=193), b"unsupported shape"),
    (dict(_NO_RES, Cout=520), b"unsupported shape"),                   # more than 8 waves x 4 column tiles
    (dict(_NO_RES, k=5, Cin=128, mid=768), b"unsupported shape"),      # no 5x5 14x14 instance with four k-steps
])
def test_mbconv_block_ex_argument_errors(change, msg):
    a = _block_ok()
    a.update(change)
    x = _lib.MbconvBlockArgs(**a)
    path = ctypes.c_int(-1)
    assert _lib.lib().mi355_mbconv_block_ex(ctypes.byref(x), ctypes.byref(path), None) != 0
    assert msg in _err(), _err()
    assert path.value == 0                                # a rejected call reports no kernel


def test_mbconv_block_ex_null_block():
    assert _lib.lib().mi355_mbconv_block_ex(None, None, None) != 0
    assert b"null" in _err()


@pytest.mark.parametrize("shape,msg", [
    ((0, 14, 96, 576, 96, 3, 1, 24, 1, 1), b"bad shape"),
    ((14, 14, 96, 576, 96, 3, 1, 0, 1, 1), b"bad shape"),
    ((14, 14, 100, 576, 96, 3, 1, 24, 1, 1), b"multiples of 8"),
    ((14, 14, 96, 576, 96, 4, 1, 24, 1, 1), b"unsupported k"),
    ((14, 14, 96, 576, 96, 3, 1, 24, 7, 1), b"activation"),
    ((14, 14, 96, 576, 96, 3, 1, 24, 1, 0), b"unsupported shape"),     # no linear-depthwise instance with three k-steps
    ((14, 15, 96, 576, 96, 3, 1, 24, 1, 1), b"unsupported shape"),
])
def test_mbconv_block_how_argument_errors(shape, msg):
    path = ctypes.c_int(-1)
    assert _lib.lib().mi355_mbconv_block_how(*shape, ctypes.byref(path)) != 0
    assert msg in _err(), _err()
    assert path.value == 0
    assert _lib.lib().mi355_mbconv_block_how(*shape, None) != 0


def test_mbconv_block_how_reports_a_path_without_a_device():
    path = ctypes.c_int(-1)
    assert _lib.lib().mi355_mbconv_block_how(14, 14, 96, 576, 96, 3, 1, 24, 1, 1, ctypes.byref(path)) == 0
    assert path.value > 0
    assert _lib.lib().mi355_mbconv_block_how(14, 14, 96, 576, 96, 3, 1, 24, 1, 1, None) == 0


def test_mbconv_block_args_layout_matches_the_header():
    F = _lib.MbconvBlockArgs
    assert ctypes.sizeof(F) == 168
    assert (F.bp.offset, F.D.offset, F.Y.offset, F.B.offset, F.Cout.offset, F.act_e.offset, F.res_n.offset, F.norot.offset) == \
        (80, 88, 96, 104, 124, 140, 160, 164)
