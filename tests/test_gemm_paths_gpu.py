"""Every branch of the GEMM dispatcher (launch_gemm_bf16, csrc/gemm_bf16.hip) against a float64 reference, op by op.

The model reaches the gated, residual, split-K and LayerNorm-folded kernels only inside residual blocks, where the block-level
tolerance cannot resolve a wrong branch (the skip connection dominates the block output).  Here each case is one call of the
developer entry mi355_gemm_bf16_ex, the call reports which branch ran, and the test asserts that it is the branch the case is
named for, so no case silently falls through to another kernel.

The reference follows the kernels' rounding points: A' = bf16(A * gate) (ReLU6 before the rounding) as in gate_chunk, then a
float64 product, the LayerNorm fold rstd (acc - mean colsum), bias, activation, residual, all in float64.  Tolerance, elementwise:
    |out - ref| <= 2^-8 |ref| + 2^-20 sum_k |A'_mk W_nk|        (one bf16 rounding of the output + fp32 accumulation)
The functions without the gpu marker check the test data alone, on CPU: a gate taken from the neighbouring image, a residual
added to all N columns instead of res_n, a missing activation and a dropped 256-deep split-K chunk must each land more than
10x the tolerance away from the reference, so the tolerance can see those bugs."""
import ctypes
import math
import os
import re
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from helpers import ROOT

DEV = "cuda:0"
BANK = 4093                 # distinct A / residual rows; row m uses bank row (m * 7919 + 13) % BANK (a permutation below BANK rows)
FULL_CHECK_ROWS = 65536     # above this: first and last 256 rows plus 4096 seeded random rows
SAMPLED = 4096
TOL_REL, TOL_ABS = 2.0 ** -8, 2.0 ** -20
MARGIN = 10.0

# include/mi355_retrieval.h (test_path_enum_matches_the_header keeps the two in step)
PATHS = {"TILE_M64_BK32": 1, "TILE_M64_BK64": 2, "TILE": 3, "BIG": 4, "BIG_KTAIL": 5, "BIG32": 6, "BIG32_KTAIL": 7, "BIG_GATED": 8,
         "BIG_GATED_KTAIL": 9, "STREAM": 10, "PROJ": 11, "SPLITK": 12, "WIDE": 13}
ACT_NONE, ACT_SILU, ACT_RELU, ACT_RELU6, ACT_GELU, ACT_SIGMOID = range(6)


@dataclass(frozen=True)
class Case:
    path: str                   # branch the shape must select
    nt: int                     # 16-column sub-tiles the branch reports (0 for kernels with a fixed tile)
    M: int
    N: int
    K: int
    act: int = ACT_NONE
    rows_per_img: int = 0       # > 0 with gate: one gate row per rows_per_img rows
    gate: bool = False
    a_relu6: bool = False
    res_n: int = 0              # > 0: residual added to the first res_n columns
    out_f32: bool = False
    ln: bool = False
    splitk: bool = False
    wide: bool = False
    lda_pad: int = 0
    ldw_pad: int = 0
    ldo_pad: int = 0
    seed: int = 0

    @property
    def lda(self):
        return self.K + self.lda_pad

    @property
    def ldw(self):
        return (self.K + 31) // 32 * 32 + self.ldw_pad

    @property
    def ldo(self):
        return self.N + self.ldo_pad

    @property
    def ldr(self):
        return (self.N + 7) // 8 * 8 if self.res_n else 0     # the residual rows are N wide; only the first res_n are added

    @property
    def n_img(self):
        return -(-self.M // self.rows_per_img) if self.rows_per_img else 1


CASES = {
    # k_gemm_bf16, M <= 64: BK = 32 below K = 64, 64 from there; every width pick_nt offers
    "tile_m64_bk32_nt2": Case("TILE_M64_BK32", 2, M=37, N=24, K=48, act=ACT_SILU, res_n=24),
    "tile_m64_bk32_nt3": Case("TILE_M64_BK32", 3, M=64, N=40, K=56, act=ACT_SIGMOID, ldo_pad=8),
    "tile_m64_bk32_nt4_f32": Case("TILE_M64_BK32", 4, M=50, N=64, K=32, act=ACT_RELU6, out_f32=True, ldo_pad=3),
    "tile_m64_bk64_nt6_gated": Case("TILE_M64_BK64", 6, M=49, N=88, K=200, act=ACT_RELU, gate=True, rows_per_img=7),
    "tile_m64_bk64_nt8_res": Case("TILE_M64_BK64", 8, M=17, N=104, K=64, act=ACT_GELU, res_n=42),
    "tile_m64_bk64_nt9_relu6": Case("TILE_M64_BK64", 9, M=64, N=136, K=96, a_relu6=True, lda_pad=8),
    "tile_m64_bk64_nt12": Case("TILE_M64_BK64", 12, M=33, N=168, K=512, act=ACT_SILU, ldw_pad=32),
    # k_gemm_bf16, 128-row tiles: gated (image boundaries inside a tile), ReLU6'd, partial residual, fp32 output, strides
    "tile_nt8_gated_res": Case("TILE", 8, M=900, N=232, K=1392, act=ACT_SILU, gate=True, rows_per_img=49, res_n=58,
                               lda_pad=8, ldw_pad=32, ldo_pad=8),
    "tile_nt3_gated_relu6_f32": Case("TILE", 3, M=500, N=40, K=96, act=ACT_RELU6, gate=True, a_relu6=True, rows_per_img=100,
                                     res_n=21, out_f32=True),
    # k_gemm_big, 64-deep stages
    "big_res_full": Case("BIG", 0, M=3000, N=200, K=256, act=ACT_GELU, res_n=200),
    "big_ktail_res_part": Case("BIG_KTAIL", 0, M=1500, N=120, K=200, act=ACT_SIGMOID, res_n=58, lda_pad=16, ldo_pad=8),
    "big_ktail_f32": Case("BIG_KTAIL", 0, M=1100, N=96, K=136, act=ACT_RELU, out_f32=True),
    "big_ln": Case("BIG", 0, M=2148, N=384, K=256, act=ACT_GELU, ln=True),
    # k_gemm_big, 32-deep stages (short K, many rows)
    "big32_k128_res": Case("BIG32", 0, M=32805, N=256, K=128, res_n=256),
    "big32_k96": Case("BIG32", 0, M=32805, N=200, K=96, act=ACT_SILU),
    "big32_ktail_k72": Case("BIG32_KTAIL", 0, M=33000, N=200, K=72, act=ACT_GELU),
    "big32_ln": Case("BIG32", 0, M=32832, N=512, K=128, ln=True),
    # k_gemm_big<GATED>: fragment-gated A, ReLU6 on A
    "big_gated": Case("BIG_GATED", 0, M=2000, N=80, K=192, gate=True, rows_per_img=196),
    "big_gated_ktail_res": Case("BIG_GATED_KTAIL", 0, M=1225, N=232, K=1392, act=ACT_SILU, gate=True, rows_per_img=49, res_n=232),
    "big_gated_relu6_only": Case("BIG_GATED", 0, M=1030, N=96, K=256, act=ACT_RELU6, a_relu6=True, res_n=48),
    "big_gated_relu6": Case("BIG_GATED", 0, M=1500, N=128, K=320, act=ACT_GELU, gate=True, a_relu6=True, rows_per_img=300),
    # k_gemm_stream (one 32-deep k-step, W resident in LDS)
    "stream_nt9_res_part": Case("STREAM", 9, M=5003, N=144, K=24, act=ACT_SILU, res_n=98, lda_pad=8),
    "stream_nt12": Case("STREAM", 12, M=4101, N=192, K=32, act=ACT_RELU6),
    # k_proj_lds (M >= 2^19, N <= 64, K <= 288)
    "proj_nt2_res": Case("PROJ", 2, M=(1 << 19) + 5, N=32, K=192, res_n=24),
    "proj_nt3_gated": Case("PROJ", 3, M=784 * 669, N=48, K=288, gate=True, rows_per_img=784),
    # split-K (256-deep chunks, reduction kernel)
    "splitk_gated_res": Case("SPLITK", 0, M=245, N=232, K=1392, act=ACT_SILU, gate=True, rows_per_img=49, res_n=232, splitk=True),
    "splitk_relu6_res_part": Case("SPLITK", 0, M=98, N=136, K=816, act=ACT_RELU, a_relu6=True, rows_per_img=49, res_n=40,
                                  splitk=True),
    # k_gemm_wide (opt-in MI355_GEMM_WIDE=1)
    "wide_res": Case("WIDE", 0, M=4098, N=264, K=160, act=ACT_GELU, res_n=264, wide=True),
    "wide_ln": Case("WIDE", 0, M=4100, N=384, K=256, ln=True, wide=True),
}


# ---------------------------------------------------------------------------------------------------------- data (CPU, seeded)
def _bank_index(rows):
    return (rows * 7919 + 13) % BANK


def _bf16(t):
    return t.to(torch.bfloat16)


class Data:
    """Seeded operands of one case.  A and the residual are banks of BANK rows that row m indexes by _bank_index(m), so the
    2^19-row cases cost no more than the small ones and any row can be rebuilt on CPU."""

    def __init__(self, c: Case):
        g = torch.Generator().manual_seed(1000 + sum(map(ord, c.path)) + c.M + 7 * c.N + 13 * c.K + c.seed)
        a_scale = 4.0 if c.a_relu6 else 0.5             # ReLU6 on A: enough values below 0 and above 6
        self.A_bank = _bf16(torch.randn(BANK, c.lda, generator=g) * a_scale)
        Np = (c.N + 15) // 16 * 16
        W = torch.zeros(Np, c.ldw)
        W[:c.N, :c.K] = torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K)
        self.W = _bf16(W)
        self.bias = torch.randn(Np, generator=g) * 0.1
        self.gate = (torch.rand(c.n_img, c.K, generator=g) * 1.2 + 0.05) if c.gate else None
        self.res_bank = _bf16(torch.randn(BANK, c.ldr, generator=g)) if c.res_n else None
        if c.ln:
            self.stats_bank = torch.stack([torch.randn(BANK, generator=g) * 0.1, torch.rand(BANK, generator=g) * 1.5 + 0.5], 1)
            self.colsum = torch.randn(Np, generator=g) * 2.0
        else:
            self.stats_bank = self.colsum = None

    def a_prime(self, c: Case, rows, gate_img=None):
        """A' rows as the kernels form them (fp32 product with the gate, ReLU6, one bf16 rounding), float64."""
        a = self.A_bank[_bank_index(rows)][:, :c.K].float()
        if c.gate:
            img = rows // c.rows_per_img if gate_img is None else gate_img
            a = a * self.gate[img]
            if c.a_relu6:
                a = a.clamp(0.0, 6.0)
            a = _bf16(a).float()
        elif c.a_relu6:
            a = a.clamp(0.0, 6.0)
        return a.double()


def _act(z, act):
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    if act == ACT_RELU:
        return z.clamp_min(0.0)
    if act == ACT_RELU6:
        return z.clamp(0.0, 6.0)
    if act == ACT_GELU:
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    return z


def reference(c: Case, d: Data, rows, mutant=None):
    """(ref, tol) at the given rows, float64; `mutant` names a deliberate bug (test_mutants_are_far_outside_the_tolerance)."""
    gate_img = None
    if mutant == "gate_from_neighbour_image":
        img = rows // c.rows_per_img
        gate_img = torch.where(img + 1 < c.n_img, img + 1, img - 1)
    a = d.a_prime(c, rows, gate_img)
    w = d.W[:c.N, :c.K].double()
    if mutant == "splitk_chunk_dropped":
        a = a.clone()
        a[:, 256:512] = 0.0                             # the second 256-deep chunk never reaches the reduction
    acc = a @ w.t()
    mag = a.abs() @ w.abs().t()
    if c.ln:
        st = d.stats_bank[_bank_index(rows)].double()
        mean, rstd = st[:, :1], st[:, 1:]
        cs = d.colsum[:c.N].double()
        acc = rstd * (acc - mean * cs)
        mag = rstd * (mag + (mean * cs).abs())
    z = acc + d.bias[:c.N].double()
    y = z if mutant == "activation_left_out" else _act(z, c.act)
    if c.res_n:
        r = d.res_bank[_bank_index(rows)].double()
        n = c.N if mutant == "residual_on_all_columns" else c.res_n
        y = y.clone()
        y[:, :n] += r[:, :n]
    tol = TOL_REL * y.abs() + TOL_ABS * mag
    return y, tol


def check_rows(c: Case):
    if c.M <= FULL_CHECK_ROWS:
        return torch.arange(c.M)
    rng = np.random.RandomState(c.M)
    pick = np.concatenate([np.arange(256), np.arange(c.M - 256, c.M), rng.randint(256, c.M - 256, SAMPLED)])
    return torch.from_numpy(np.unique(pick))


MUTANTS = {
    "gate_from_neighbour_image": lambda c: c.gate,
    "residual_on_all_columns": lambda c: 0 < c.res_n < c.N,
    "activation_left_out": lambda c: c.act != ACT_NONE,
    "splitk_chunk_dropped": lambda c: c.splitk,
}


def test_every_dispatch_branch_has_a_case():
    assert {c.path for c in CASES.values()} == set(PATHS)
    assert {c.act for c in CASES.values()} == set(range(6))
    m64 = {c.nt for c in CASES.values() if c.path.startswith("TILE")}
    assert m64 == {2, 3, 4, 6, 8, 9, 12}
    for mut, applies in MUTANTS.items():
        assert any(applies(c) for c in CASES.values()), mut


def test_path_enum_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"MI355_GEMM_PATH_([A-Z0-9_]+)\s*=\s*(\d+)", txt)}
    assert got == PATHS


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if any(a(c) for a in MUTANTS.values())])
def test_mutants_are_far_outside_the_tolerance(name):
    """CPU only: on this case's data each applicable bug moves some output more than MARGIN x its tolerance."""
    c = CASES[name]
    d = Data(c)
    rows = check_rows(c)
    ref, tol = reference(c, d, rows)
    for mut, applies in MUTANTS.items():
        if not applies(c):
            continue
        m, _ = reference(c, d, rows, mut)
        ratio = ((m - ref).abs() / tol).max().item()
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture
def gemm_wide_env():
    """MI355_GEMM_WIDE is read per call by launch_gemm_bf16; leave the process as it was found."""
    old = os.environ.get("MI355_GEMM_WIDE")
    yield lambda v: os.environ.__setitem__("MI355_GEMM_WIDE", v)
    if old is None:
        os.environ.pop("MI355_GEMM_WIDE", None)
    else:
        os.environ["MI355_GEMM_WIDE"] = old


def _splitk_bytes(c):
    return -(-c.K // 256) * c.M * ((c.N + 15) // 16 * 16) * 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gemm_branch_matches_float64(name, gemm_wide_env):
    from imageretrievalresearch_amd._lib import GemmExArgs, check, lib, stream_ptr
    c = CASES[name]
    d = Data(c)
    idx = _bank_index(torch.arange(c.M)).to(DEV)
    A = d.A_bank.to(DEV)[idx].contiguous()
    W = d.W.to(DEV)
    bias = d.bias.to(DEV)
    keep = [A, W, bias]
    x = GemmExArgs(A=A.data_ptr(), lda=c.lda, W=W.data_ptr(), ldw=c.ldw, bias=bias.data_ptr(), M=c.M, N=c.N, K=c.K, act=c.act,
                   ldo=c.ldo, out_f32=int(c.out_f32), a_relu6=int(c.a_relu6), rows_per_img=c.rows_per_img)
    if c.res_n:
        res = d.res_bank.to(DEV)[idx].contiguous()
        keep.append(res)
        x.res, x.ldr, x.res_n = res.data_ptr(), c.ldr, c.res_n
    if c.gate:
        gate = d.gate.to(DEV)
        keep.append(gate)
        x.gate, x.gate_ld = gate.data_ptr(), c.K
    if c.ln:
        stats = d.stats_bank.to(DEV)[idx].contiguous()
        colsum = d.colsum.to(DEV)
        keep += [stats, colsum]
        x.ln_stats, x.ln_colsum = stats.data_ptr(), colsum.data_ptr()
    if c.splitk:
        ws = torch.empty(_splitk_bytes(c) // 4, device=DEV)
        keep.append(ws)
        x.splitk_ws, x.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
    sentinel = float("nan")
    out = torch.full((c.M, c.ldo), sentinel, device=DEV, dtype=torch.float32 if c.out_f32 else torch.bfloat16)
    x.out = out.data_ptr()
    gemm_wide_env("1" if c.wide else "0")
    path = ctypes.c_int(-1)
    check(lib().mi355_gemm_bf16_ex(ctypes.byref(x), ctypes.byref(path), stream_ptr(DEV)))
    torch.cuda.synchronize()
    kind, nt = path.value & 0xff, (path.value >> 8) & 0xff
    assert (kind, nt) == (PATHS[c.path], c.nt), f"{name}: ran path {kind} nt {nt}, expected {c.path} nt {c.nt}"
    rows = check_rows(c)
    got = out[rows.to(DEV)].cpu()
    assert torch.isnan(got[:, c.N:].float()).all(), f"{name}: wrote past N into the ldo padding"
    got = got[:, :c.N].double()
    ref, tol = reference(c, d, rows)
    assert torch.isfinite(got).all(), f"{name}: non-finite or unwritten outputs"
    ratio = ((got - ref).abs() / tol)
    worst = ratio.max().item()
    print(f"gemm {name:28s} path {c.path:16s} M={c.M} N={c.N} K={c.K}: worst |err| / tol = {worst:.3f}")
    assert worst <= 1.0, f"{name}: worst |err| / tol {worst:.3f} at {np.unravel_index(ratio.argmax().item(), ratio.shape)}"
