"""The developer entries mi355_stem_ex, mi355_head_gap_ex, mi355_gap, mi355_nhwc_to_nchw and mi355_nchw_to_nhwc, the parts that
need no GPU: the C-ABI symbols, every argument check (rejected before any HIP call, with a message), and the float64 references of
tests/stem_head_ref.py themselves: each modelled bug must move some output of each case it applies to by more than 10x the
tolerance on the case's own data, and the reference stem is pinned against torch.nn.functional.conv2d and oracle.common.fold_bn."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import stem_head_ref as R
from helpers import ROOT, header_symbols
from imageretrievalresearch_amd import _lib

NEW = ["mi355_stem_ex", "mi355_head_gap_ex", "mi355_gap", "mi355_nhwc_to_nchw", "mi355_nchw_to_nhwc"]
P = 1 << 20          # a 16-byte aligned stand-in pointer: nothing is dereferenced when a check fails
MARGIN = 10.0


def _err():
    return _lib.lib().mi355_last_error()


def test_symbols_declared_bound_and_exported():
    for name in NEW + ["mi355_pool_linear"]:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib().mi355_abi_version() == 3


def test_path_enums_match_the_header():
    txt = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    got = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"MI355_STEM_PATH_([A-Z0-9_]+)\s*=\s*(0x[0-9a-f]+|\d+)", txt)}
    assert got == R.STEM_PATHS
    assert "#define MI355_HEAD_GAP_PATH(act, ksmax) ((act) | (ksmax) << 8)" in txt
    assert R.HEAD_CASES["k416_ksmax16"].path == 1 | 16 << 8 and R.HEAD_CASES["k32_hw64_b5"].path == 0 | 12 << 8


def test_stem_ex_args_layout_matches_the_header():
    S = _lib.StemExArgs
    assert ctypes.sizeof(S) == 112
    assert (S.images_bytes.offset, S.B.offset, S.fill.offset, S.mean.offset, S.conv_input_w.offset, S.out.offset, S.Cout.offset,
            S.act.offset) == (16, 40, 52, 56, 72, 96, 104, 108)


# --------------------------------------------------------------------------------------------------------------- refusals
_MEAN = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
_STD = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
_STD0 = (ctypes.c_float * 3)(0.229, 0.0, 0.225)


def _stem_f32():
    return dict(x=P, B=2, H=32, W=32, w=P, bias=P, out=P, Cout=40, act=1)


def _stem_u8():
    return dict(images=P, B=2, H=33, W=20, fill=255, mean=_MEAN, stdv=_STD, w=P, bias=P, out=P, Cout=40, act=1)


def _desc(rows):
    return (ctypes.c_int64 * (3 * len(rows)))(*[v for r in rows for v in r])


_D_OK = _desc([(0, 66, 10), (1980, 66, 66)])
_D_SHORT = _desc([(0, 66, 10), (1980, 60, 66 - 2)])
_D_OUTSIDE = _desc([(0, 66, 10), (1980, 66, 67)])


def _stem_ragged(d=_D_OK):
    return dict(_stem_u8(), H=66, W=66, images_bytes=1980 + 66 * 66 * 3, desc_host=ctypes.addressof(d), desc_dev=P)


@pytest.mark.parametrize("base,change,msg", [
    (_stem_f32, dict(w=None), b"null"),
    (_stem_f32, dict(bias=None), b"null"),
    (_stem_f32, dict(out=None), b"null"),
    (_stem_f32, dict(x=None), b"exactly one"),
    (_stem_f32, dict(images=P), b"exactly one"),
    (_stem_f32, dict(B=0), b"bad shape"),
    (_stem_f32, dict(B=65536), b"bad shape"),
    (_stem_f32, dict(H=0), b"bad shape"),
    (_stem_f32, dict(W=-4), b"bad shape"),
    (_stem_f32, dict(W=16388), b"bad shape"),
    (_stem_f32, dict(Cout=0), b"multiple of 8"),
    (_stem_f32, dict(Cout=36), b"multiple of 8"),
    (_stem_f32, dict(Cout=264), b"multiple of 8"),
    (_stem_f32, dict(act=6), b"activation"),
    (_stem_f32, dict(act=-1), b"activation"),
    (_stem_f32, dict(x=P + 4), b"16-byte aligned"),
    (_stem_f32, dict(w=P + 8), b"16-byte aligned"),
    (_stem_f32, dict(bias=P + 4), b"16-byte aligned"),
    (_stem_f32, dict(out=P + 2), b"16-byte aligned"),
    (_stem_f32, dict(conv_input_w=P), b"belong to the uint8 form"),
    (_stem_f32, dict(desc_dev=P), b"belong to the uint8 form"),
    (_stem_u8, dict(mean=None), b"null"),
    (_stem_u8, dict(stdv=None), b"null"),
    (_stem_u8, dict(fill=256), b"fill"),
    (_stem_u8, dict(fill=-1), b"fill"),
    (_stem_u8, dict(stdv=_STD0), b"std[1] is zero"),
    (_stem_u8, dict(conv_input_w=P + 2), b"4-byte aligned"),
    (_stem_u8, dict(desc_dev=P), b"go together"),
    (_stem_u8, dict(desc_host=ctypes.addressof(_D_OK)), b"go together"),
    (_stem_u8, dict(Cout=12), b"multiple of 8"),
    (_stem_ragged, dict(H=66, W=64), b"H == W == S"),
    (_stem_ragged, dict(H=70, W=70), b"longer side"),
    (lambda: _stem_ragged(_D_SHORT), dict(), b"longer side"),
    (lambda: _stem_ragged(_D_OUTSIDE), dict(), b"stem_ex"),            # the second image ends past images_bytes
    (_stem_ragged, dict(images_bytes=1980), b"stem_ex"),
])
def test_stem_ex_argument_errors(base, change, msg):
    a = base()
    a.update(change)
    x = _lib.StemExArgs(**a)
    path = ctypes.c_int(-1)
    assert _lib.lib().mi355_stem_ex(ctypes.byref(x), ctypes.byref(path), None) != 0
    assert msg in _err(), _err()
    assert path.value == 0                                # a rejected call reports no kernel


def test_stem_ex_null_block():
    assert _lib.lib().mi355_stem_ex(None, None, None) != 0
    assert b"null" in _err()


def _hg():
    """A valid head + GAP call (B = 4, HW = 49, N = 136, K = 384) with stand-in pointers."""
    return dict(A=P, lda=384, W=P, ldw=384, bias=P, pooled=P, pooled_bf16=P, ldp=136, B=4, HW=49, N=136, K=384, act=1)


_HG_ORDER = ["A", "lda", "W", "ldw", "bias", "pooled", "pooled_bf16", "ldp", "B", "HW", "N", "K", "act"]


@pytest.mark.parametrize("change,msg", [
    (dict(A=None), b"null"),
    (dict(W=None), b"null"),
    (dict(bias=None), b"null"),
    (dict(pooled=None), b"null"),
    (dict(B=0), b"bad shape"),
    (dict(N=0), b"bad shape"),
    (dict(HW=0), b"1 <= HW <= 64"),
    (dict(HW=65), b"1 <= HW <= 64"),
    (dict(K=24, lda=24, ldw=32), b"32 <= K <= 512"),
    (dict(K=520, lda=520, ldw=544), b"32 <= K <= 512"),
    (dict(lda=380), b"lda a multiple of 8"),
    (dict(lda=376), b"lda a multiple of 8"),             # a multiple of 8, but below K
    (dict(ldw=376), b"ldw a multiple of 32"),
    (dict(K=392, lda=392, ldw=392), b"ldw a multiple of 32"),
    (dict(K=392, lda=392, ldw=384), b"ldw a multiple of 32"),
    (dict(N=132), b"N a multiple of 8"),
    (dict(act=2), b"act none or SiLU"),
    (dict(act=4), b"act none or SiLU"),
    (dict(ldp=128), b"ldp"),
    (dict(ldp=137), b"ldp"),
    (dict(A=P + 8), b"aligned"),
    (dict(pooled=P + 4), b"aligned"),
    (dict(pooled_bf16=P + 2), b"aligned"),
])
def test_head_gap_ex_argument_errors(change, msg):
    a = _hg()
    a.update(change)
    path = ctypes.c_int(-1)
    assert _lib.lib().mi355_head_gap_ex(*[a[k] for k in _HG_ORDER], ctypes.byref(path), None) != 0
    assert msg in _err(), _err()
    assert path.value == 0


@pytest.mark.parametrize("args,msg", [
    ((None, 2, 49, 64, P, P), b"null"),
    ((P, 2, 49, 64, None, P), b"null"),
    ((P, 0, 49, 64, P, P), b"bad shape"),
    ((P, 2, 0, 64, P, P), b"bad shape"),
    ((P, 2, 49, 0, P, P), b"bad shape"),
    ((P, 2, 49, 60, P, P), b"multiple of 8"),
    ((P + 8, 2, 49, 64, P, P), b"aligned"),
    ((P, 2, 49, 64, P + 4, P), b"aligned"),
    ((P, 2, 49, 64, P, P + 2), b"aligned"),
])
def test_gap_argument_errors(args, msg):
    assert _lib.lib().mi355_gap(*args, None) != 0
    assert msg in _err(), _err()


@pytest.mark.parametrize("fn", ["mi355_nhwc_to_nchw", "mi355_nchw_to_nhwc"])
@pytest.mark.parametrize("args,msg", [
    ((None, P, 2, 49, 40, 40), b"null"),
    ((P, None, 2, 49, 40, 40), b"null"),
    ((P, P, 0, 49, 40, 40), b"bad shape"),
    ((P, P, 65536, 49, 40, 40), b"bad shape"),
    ((P, P, 2, 0, 40, 40), b"bad shape"),
    ((P, P, 2, 49, 0, 0), b"bad shape"),
    ((P, P, 2, 49, 40, 0), b"Cvalid"),
    ((P, P, 2, 49, 40, 41), b"Cvalid"),
    ((P + 1, P, 2, 49, 40, 40), b"aligned"),
    ((P, P + 1, 2, 49, 40, 40), b"aligned"),
])
def test_layout_argument_errors(fn, args, msg):
    assert getattr(_lib.lib(), fn)(*args, None) != 0
    assert msg in _err(), _err()
    assert fn[6:].encode() in _err()


def test_layout_alignment_is_the_element_size():
    """The fp32 side needs 4 bytes, the bf16 side 2: a pointer that suits bf16 only is refused on the fp32 side."""
    L = _lib.lib()
    assert L.mi355_nhwc_to_nchw(P, P + 2, 2, 49, 40, 40, None) != 0 and b"aligned" in _err()
    assert L.mi355_nchw_to_nhwc(P + 2, P, 2, 49, 40, 40, None) != 0 and b"aligned" in _err()


# ------------------------------------------------------------------------------------------------------------- references
def test_bf16_helpers_match_torch():
    rng = np.random.RandomState(1)
    x = np.concatenate([R.SPECIALS, rng.standard_normal(4096).astype(np.float32),
                        rng.randint(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(R.bf16_bits(x), R.canon_nan(want))
    assert np.isnan(x).sum() > 8 and np.array_equal(np.isnan(R.bf16_to_f32(want)), np.isnan(x))
    back = torch.from_numpy(want.view(np.int16)).view(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(R.bf16_to_f32(want).view(np.uint32), back.view(np.uint32))
    # the data of the layout tests holds what the issue lists: both zeros, denormals, both infinities, a NaN, halfway cases of
    # both parities and the largest fp32, which rounds to Inf
    b = R.bf16_bits(R.SPECIALS)
    assert {0x0000, 0x8000, 0x7f80, 0xff80, 0x7fc0} <= set(b.tolist())
    assert R.bf16_bits(np.array([0x3f808000, 0x3f818000], np.uint32).view(np.float32)).tolist() == [0x3f80, 0x3f82]
    assert R.bf16_bits(np.array([0x7f7fffff], np.uint32).view(np.float32)).tolist() == [0x7f80]


@pytest.mark.parametrize("name", list(R.STEM_CASES))
def test_reference_stem_matches_torch_conv2d_and_fold_bn(name):
    from oracle.common import Rounder, fold_bn
    c = R.STEM_CASES[name]
    d = R.StemData(c)
    g, beta, mean, var = (torch.from_numpy(t) for t in d.bn)
    w, b = fold_bn(torch.from_numpy(d.w_raw), dict(weight=g, bias=beta, running_mean=mean, running_var=var), R.BN_EPS)
    w = Rounder(True)(w)                                                       # [Cout][ci][ky][kx], bf16 values
    assert torch.equal(w.permute(2, 3, 1, 0).reshape(27, c.Cout), torch.from_numpy(d.w)), name
    assert torch.equal(b, torch.from_numpy(d.bias)), name
    z = torch.nn.functional.conv2d(torch.from_numpy(d.x).double(), w.double(), b.double(), stride=2, padding=1)
    y, mag = R.stem(d.x, d.w, d.bias, R.ACT_NONE)
    np.testing.assert_allclose(y, z.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    zm = torch.nn.functional.conv2d(torch.from_numpy(d.x).double().abs(), w.double().abs(), b.double().abs(), stride=2, padding=1)
    np.testing.assert_allclose(mag, zm.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    assert y.shape == (c.B, (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1, c.Cout)


def test_reference_preprocess_and_conv_input_match_the_oracle():
    from oracle import preprocess as opre
    c = R.U8_CASES["ci_33x20"]
    d = R.U8Data(c, "ci_33x20")
    for fill in (255, 0, 37):
        np.testing.assert_array_equal(R.preprocess(d.imgs[1], fill, opre.MEAN, opre.STD),
                                      opre.to_tensor_normalize(opre.square_pad(d.imgs[1], fill)))
    Pre = np.stack([R.preprocess(im, c.fill, c.mean, c.std) for im in d.imgs])
    want = torch.nn.functional.conv2d(torch.from_numpy(Pre).double(), torch.from_numpy(d.cw).double(), padding=1)
    got, _ = R.conv_input_silu(Pre, d.cw)
    np.testing.assert_allclose(got, torch.nn.functional.silu(want).numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", list(R.STEM_CASES))
def test_stem_mutants_are_far_outside_the_tolerance(name):
    c = R.STEM_CASES[name]
    d = R.StemData(c)
    y, mag = R.stem(d.x, d.w, d.bias, c.act)
    tol = R.stem_tol(y, mag)
    for mut, applies in R.STEM_MUTANTS.items():
        if not applies(c):
            continue
        m, _ = R.stem(d.x, d.w, d.bias, c.act, mut)
        ratio = (np.abs(m - y) / tol).max()
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


@pytest.mark.parametrize("name", list(R.U8_CASES))
def test_u8_mutants_are_far_outside_the_tolerance(name):
    c = R.U8_CASES[name]
    d = R.U8Data(c, name)
    y, tol = d.reference(c)
    assert np.isfinite(y).all() and (tol > 0).all()
    for mut, applies in R.U8_MUTANTS.items():
        if not applies(c):
            continue
        m, _ = d.reference(c, mut)
        ratio = (np.abs(m - y) / tol).max()
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


def test_every_u8_instantiation_and_setting_has_a_case():
    cs = R.U8_CASES.values()
    assert {(c.conv_input, c.ragged) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
    for ci in (False, True):
        mine = [c for c in cs if c.conv_input == ci]
        assert {c.fill for c in mine} == {255, 0, 37}
        assert any(c.mean != (0.485, 0.456, 0.406) for c in mine)
        assert {c.sizes[0] for c in mine if not c.ragged} == {(64, 64), (33, 20), (41, 70), (1, 1)}
        assert [c.sizes for c in mine if c.ragged] == [((66, 10), (66, 66), (3, 66), (65, 66))]
    for c in cs:
        assert len({max(s) for s in c.sizes}) == 1
    for mut, applies in R.U8_MUTANTS.items():
        assert any(applies(c) for c in cs), mut


@pytest.mark.parametrize("name", list(R.HEAD_CASES))
def test_head_gap_mutants_are_far_outside_the_tolerance(name):
    c = R.HEAD_CASES[name]
    d = R.HeadData(c)
    ref, tol = d.reference(c)
    for mut in R.HEAD_MUTANTS:
        if not R.head_mutant_applies(mut, c):
            continue
        m, _ = d.reference(c, mut)
        ratio = (np.abs(m - ref) / tol).max()
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


def test_every_head_and_pool_mutant_has_a_case():
    for mut in R.HEAD_MUTANTS:
        assert any(R.head_mutant_applies(mut, c) for c in R.HEAD_CASES.values()), mut
    assert {c.path for c in R.HEAD_CASES.values()} == {a | k << 8 for a in (0, 1) for k in (12, 16)} - {0 | 16 << 8} | \
        {R.HEAD_CASES["k512_hw30"].path}


@pytest.mark.parametrize("B,HW,C", R.GAP_CASES)
def test_gap_mutants_are_far_outside_the_tolerance(B, HW, C):
    x = R.gap_data(B, HW, C)
    ref, tol = R.pool(x), R.pool_tol(x)
    for mut, applies in R.POOL_MUTANTS.items():
        if applies(B, HW):
            ratio = (np.abs(R.pool(x, mut) - ref) / tol).max()
            assert ratio > MARGIN, f"gap {(B, HW, C)}: mutant {mut} only {ratio:.1f}x the tolerance"


@pytest.mark.parametrize("B,C,HW,N,has_bias", R.POOL_LINEAR_CASES)
def test_pool_linear_mutants_are_far_outside_the_tolerance(B, C, HW, N, has_bias):
    fm, w, bias = R.pool_linear_data(B, C, HW, N, has_bias)
    x = fm.transpose(0, 2, 1)                                              # [B][HW][C]
    ref, tol = R.pool(x), R.pool_tol(x)
    for mut, applies in R.POOL_MUTANTS.items():
        if not applies(B, HW):
            continue
        m = R.pool(x, mut)
        ratio = (np.abs(m - ref) / tol).max()
        assert ratio > MARGIN, f"pool_linear {(B, C, HW, N)}: mutant {mut} only {ratio:.1f}x the tolerance (pooled)"
        if N:       # and the Linear on the wrong pooled values is far outside the Linear's tolerance too
            out, otol = R.pool_linear_out(ref.astype(np.float32), w, bias)
            mout, _ = R.pool_linear_out(m.astype(np.float32), w, bias)
            ratio = (np.abs(mout - out) / otol).max()
            assert ratio > MARGIN, f"pool_linear {(B, C, HW, N)}: mutant {mut} only {ratio:.1f}x the tolerance (out)"


@pytest.mark.parametrize("B,HW,C,Cvalid", R.LAYOUT_CASES)
def test_layout_references(B, HW, C, Cvalid):
    x = R.layout_data(B, HW, C, Cvalid, seed=B + HW + C)
    bits = R.nchw_to_nhwc(x, B, HW, C, Cvalid)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)       # [B][Cvalid][HW]
    np.testing.assert_array_equal(bits[:, :, :Cvalid], R.canon_nan(want).transpose(0, 2, 1))
    assert not bits[:, :, Cvalid:].any()
    back = R.nhwc_to_nchw(bits, B, HW, C, Cvalid)
    np.testing.assert_array_equal(R.bf16_bits(back).reshape(B, Cvalid, HW), R.canon_nan(want))    # the round trip keeps the bits
    if Cvalid < C:      # exact tests: any difference is outside the tolerance
        assert not np.array_equal(R.nchw_to_nhwc(x, B, HW, C, Cvalid, "cvalid_ignored"), bits)
        full = R.bf16_bits(R.layout_data(B, HW, C, C, seed=1)).transpose(0, 2, 1).copy()
        good, bad = (np.full(B * Cvalid * HW + R.GUARD, np.nan, np.float32) for _ in range(2))     # output buffer + NaN guard
        good[:B * Cvalid * HW] = R.nhwc_to_nchw(full, B, HW, C, Cvalid)
        m = R.nhwc_to_nchw(full, B, HW, C, Cvalid, "cvalid_ignored")[:bad.size]
        bad[:m.size] = m
        assert not np.array_equal(bad.view(np.uint32), good.view(np.uint32))      # wrong values, or a write into the guard
    assert any(cv < c for _, _, c, cv in R.LAYOUT_CASES)
