"""The developer entries mi355_window_attention and mi355_gemm_bf16_ex, the parts that need no GPU: the C-ABI symbols and
every argument check (rejected before any HIP call, with a message)."""
import ctypes

import pytest

from helpers import header_symbols
from imageretrievalresearch_amd import _lib

NEW = ["mi355_window_attention", "mi355_gemm_bf16_ex"]
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
