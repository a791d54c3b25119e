"""The developer entries mi355_swin_layernorm, mi355_swin_patch_embed and mi355_swin_ln_token_mean, the parts that need no GPU:
the C-ABI symbols and every argument check (rejected before any HIP call, with a message)."""
import ctypes

import pytest

from helpers import header_symbols
from imageretrievalresearch_amd import _lib

NEW = ["mi355_swin_layernorm", "mi355_swin_patch_embed", "mi355_swin_ln_token_mean"]
P = 1 << 20          # a 16-byte aligned stand-in pointer: nothing is dereferenced when a check fails
F3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_declared_bound_and_exported():
    for name in NEW:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib().mi355_abi_version() == 3


def _ln_ok():
    """A valid call (2 images of 3x5 merged tokens, C = 512) with stand-in pointers."""
    return dict(in_=P, gamma=P, beta=P, out=P, rows=30, C=512, merge=1, gh=3, gw=5, stats=0, eps=1e-5)


@pytest.mark.parametrize("change,msg", [
    (dict(in_=None), b"null"),
    (dict(out=None), b"null"),
    (dict(gamma=None), b"null"),
    (dict(beta=None), b"null"),
    (dict(merge=0, stats=1, in_=None, gamma=None, beta=None), b"null"),     # stats needs no gamma / beta, but its input
    (dict(merge=2), b"0 or 1"),
    (dict(stats=-1), b"0 or 1"),
    (dict(stats=1), b"merge with stats"),
    (dict(C=64), b"unsupported width"),
    (dict(C=640), b"unsupported width"),
    (dict(C=0), b"unsupported width"),
    (dict(C=4096), b"unsupported width"),
    (dict(rows=0), b"bad shape"),
    (dict(rows=-15), b"bad shape"),
    (dict(rows=1 << 31, merge=0), b"bad shape"),
    (dict(gh=0), b"bad shape"),
    (dict(gw=-5), b"bad shape"),
    (dict(rows=31), b"multiple of gh * gw"),
    (dict(rows=15, gh=5, gw=5), b"multiple of gh * gw"),
    (dict(eps=0.0), b"eps"),
    (dict(eps=-1e-5), b"eps"),
    (dict(in_=P + 8), b"aligned"),
    (dict(out=P + 2), b"aligned"),
    (dict(gamma=P + 4), b"aligned"),
    (dict(beta=P + 8), b"aligned"),
])
def test_layernorm_argument_errors(change, msg):
    a = _ln_ok()
    a.update(change)
    assert _lib.lib().mi355_swin_layernorm(a["in_"], a["gamma"], a["beta"], a["out"], a["rows"], a["C"], a["merge"], a["gh"], a["gw"],
                                           a["stats"], a["eps"], None) != 0
    assert msg in _err(), _err()


def _pe_ok():
    """A valid fp32 call (B = 2, H = 12, embed 128) with stand-in pointers; _U8 / _RAGGED turn it into the uint8 modes."""
    return dict(x=P, images=None, desc=None, b0=0, B=2, H=12, h=0, w=0, fill=0, mean=None, stdv=None, weight=P, bias=P, gamma=P, beta=P,
                embed=128, eps=1e-5, out=P)


_U8 = dict(x=None, images=P, H=224, h=224, w=150, fill=255, mean=F3, stdv=F3)
_RAGGED = dict(_U8, desc=P, b0=1, h=0, w=0)


@pytest.mark.parametrize("change,msg", [
    (dict(x=None), b"exactly one of x and images"),
    (dict(images=P), b"exactly one of x and images"),
    (dict(weight=None), b"null"),
    (dict(bias=None), b"null"),
    (dict(gamma=None), b"null"),
    (dict(beta=None), b"null"),
    (dict(out=None), b"null"),
    (dict(_U8, mean=None), b"null"),
    (dict(_U8, stdv=None), b"null"),
    (dict(embed=64), b"128 or 96"),
    (dict(embed=192), b"128 or 96"),
    (dict(B=0), b"bad shape"),
    (dict(B=70000), b"bad shape"),
    (dict(H=10), b"multiple of 4"),
    (dict(H=0), b"multiple of 4"),
    (dict(H=228), b"multiple of 4"),
    (dict(desc=P), b"desc_dev goes with images"),
    (dict(_U8, H=112), b"224 x 224 square"),
    (dict(_U8, h=200, w=150), b"longer side must be 224"),
    (dict(_U8, h=224, w=300), b"longer side must be 224"),
    (dict(_U8, h=224, w=0), b"longer side must be 224"),
    (dict(_U8, fill=256), b"fill"),
    (dict(_U8, fill=-1), b"fill"),
    (dict(_RAGGED, b0=-1), b"negative"),
    (dict(eps=0.0), b"eps"),
    (dict(x=P + 4), b"aligned"),
    (dict(out=P + 8), b"aligned"),
    (dict(bias=P + 4), b"aligned"),
    (dict(gamma=P + 8), b"aligned"),
    (dict(beta=P + 4), b"aligned"),
    (dict(weight=P + 2), b"aligned"),
    (dict(_RAGGED, desc=P + 4), b"aligned"),
])
def test_patch_embed_argument_errors(change, msg):
    a = _pe_ok()
    a.update(change)
    assert _lib.lib().mi355_swin_patch_embed(a["x"], a["images"], a["desc"], a["b0"], a["B"], a["H"], a["h"], a["w"], a["fill"], a["mean"],
                                             a["stdv"], a["weight"], a["bias"], a["gamma"], a["beta"], a["embed"], a["eps"], a["out"],
                                             None) != 0
    assert msg in _err(), _err()


def _tm_ok():
    return dict(in_=P, gamma=P, beta=P, pooled=P, pooled_bf16=P, B=3, L=49, C=1024, eps=1e-5)


@pytest.mark.parametrize("change,msg", [
    (dict(in_=None), b"null"),
    (dict(gamma=None), b"null"),
    (dict(beta=None), b"null"),
    (dict(pooled=None), b"null"),
    (dict(pooled_bf16=None), b"null"),
    (dict(C=512), b"unsupported width"),
    (dict(C=1536), b"unsupported width"),
    (dict(L=0), b"bad shape"),
    (dict(L=-49), b"bad shape"),
    (dict(B=0), b"bad shape"),
    (dict(B=1 << 20, L=1 << 20), b"too large"),
    (dict(eps=0.0), b"eps"),
    (dict(in_=P + 8), b"aligned"),
    (dict(gamma=P + 2), b"aligned"),
    (dict(beta=P + 1), b"aligned"),
    (dict(pooled=P + 2), b"aligned"),
    (dict(pooled_bf16=P + 1), b"aligned"),
])
def test_ln_token_mean_argument_errors(change, msg):
    a = _tm_ok()
    a.update(change)
    assert _lib.lib().mi355_swin_ln_token_mean(a["in_"], a["gamma"], a["beta"], a["pooled"], a["pooled_bf16"], a["B"], a["L"], a["C"],
                                               a["eps"], None) != 0
    assert msg in _err(), _err()
