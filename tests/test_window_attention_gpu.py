"""Swin window attention (k_win_attn, csrc/swin_kernels.hip) on its own, against a float64 reference.

The block-level Swin tests compare whole residual blocks with a relative L2 sized for bf16 rounding; the attention branch is only
a part of a block's output, so a missing or transposed relative-position bias, a dropped key or a missing shift mask can stay
under that tolerance.  Here one attention layer runs through the developer entry mi355_window_attention, which packs the
(169, heads) bias table with the model's own packing routine and launches the model's kernel.

The reference is float64, built from the exact bf16 qkv values with oracle/swin.py's window_partition, relative_position_index,
attn_mask and torch.roll (timm's formulation, not the kernel's region labels).  Tolerance, elementwise:
    |o - ref| <= 2^-8 max_key |v| + 2^-8 |ref|
(P rounded to bf16 before P V, the bf16 output, the exp2 / rcp approximations).  The functions without the gpu marker check the
data alone, on CPU: each deliberate bug below must move some output more than 10x its tolerance."""
import math

import numpy as np
import pytest
import torch

from oracle import swin

DEV = "cuda:0"
WS, NTOK, HD = 7, 49, 32
TOL = 2.0 ** -8
MARGIN = 10.0

# name -> (B, res, heads, shift, kind); kind picks the data (see make_data)
CASES = {
    "stage1_res56_h4": (1, 56, 4, 0, "normal"),
    "stage1_res56_h4_shift": (1, 56, 4, 3, "normal"),
    "stage2_res28_h8": (1, 28, 8, 0, "normal"),
    "stage2_res28_h8_shift": (1, 28, 8, 3, "normal"),
    "stage3_res14_h16": (1, 14, 16, 0, "normal"),
    "stage3_res14_h16_shift": (1, 14, 16, 3, "normal"),
    "stage4_res7_h32": (1, 7, 32, 0, "normal"),
    "batch3_res14_h16_shift": (3, 14, 16, 3, "normal"),
    "batch2_res28_h8_shift": (2, 28, 8, 3, "normal"),
    "peaked_res28_h8_shift": (1, 28, 8, 3, "peaked"),
    "identical_keys_res14_h16_shift": (2, 14, 16, 3, "identical_keys"),
    "large_table_res14_h16_shift": (1, 14, 16, 3, "large_table"),
    "large_table_res7_h32": (2, 7, 32, 0, "large_table"),
}


def make_data(name):
    """(qkv bf16 [B][res*res][3C], bias table fp32 [169][heads]), seeded per case."""
    B, res, heads, shift, kind = CASES[name]
    C = HD * heads
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    qkv = torch.randn(B, res * res, 3 * C, generator=g)
    table = torch.randn((2 * WS - 1) ** 2, heads, generator=g) * 0.5
    if kind == "peaked":
        # scale q and k so that the largest logit is about 30: softmax close to one-hot
        q, k = qkv[..., :C].bfloat16().double(), qkv[..., C:2 * C].bfloat16().double()
        mx = _max_logit(q, k, B, res, heads)
        qkv[..., :2 * C] *= math.sqrt(30.0 / mx)
    elif kind == "identical_keys":
        qkv[..., C:2 * C] = qkv[0, 0, C:2 * C]            # every key of every head is the same vector
        table = table * 4.0                               # the bias alone shapes the softmax: give it room
    elif kind == "large_table":
        table = torch.randn((2 * WS - 1) ** 2, heads, generator=g) * 8.0
    return qkv.bfloat16(), table.float()


def _max_logit(q, k, B, res, heads):
    qw = swin.window_partition(q.view(B, res, res, -1), WS).view(-1, NTOK, heads, HD).transpose(1, 2)
    kw = swin.window_partition(k.view(B, res, res, -1), WS).view(-1, NTOK, heads, HD).transpose(1, 2)
    return float((qw @ kw.transpose(-1, -2)).abs().max()) * HD ** -0.5


MUTANTS = ["bias_left_out", "bias_transposed", "last_key_dropped", "shift_mask_left_out", "shift_reversed", "scale_left_out"]


def applicable(name, mutant):
    _, _, _, shift, kind = CASES[name]
    if mutant in ("shift_mask_left_out", "shift_reversed"):
        return shift > 0
    if mutant == "scale_left_out":
        return kind != "identical_keys"        # q.k is the same for every key of a query: the scale cancels in the softmax
    return True


def reference(name, qkv, table, mutant=None):
    """(ref, tol) [B][res*res][C] float64.  `mutant` names a deliberate bug (test_mutants_are_far_outside_the_tolerance)."""
    B, res, heads, shift, _ = CASES[name]
    C = HD * heads
    x = qkv.double().view(B, res, res, 3 * C)
    fwd, back = (shift, -shift) if mutant == "shift_reversed" else (-shift, shift)
    if shift:
        x = torch.roll(x, shifts=(fwd, fwd), dims=(1, 2))
    win = swin.window_partition(x, WS).view(-1, NTOK, 3, heads, HD).permute(2, 0, 3, 1, 4)   # [3][Bw][heads][49][32]
    q, k, v = win[0], win[1], win[2]
    scale = 1.0 if mutant == "scale_left_out" else HD ** -0.5
    attn = (q * scale) @ k.transpose(-2, -1)
    if mutant != "bias_left_out":
        bias = table.double()[swin.relative_position_index().view(-1)].view(NTOK, NTOK, heads).permute(2, 0, 1)   # [h][q][k]
        if mutant == "bias_transposed":
            bias = bias.transpose(1, 2)
        attn = attn + bias.unsqueeze(0)
    if shift and mutant != "shift_mask_left_out":
        m = swin.attn_mask(res, res, WS, shift).double()
        nW = m.shape[0]
        attn = (attn.view(-1, nW, heads, NTOK, NTOK) + m.unsqueeze(1).unsqueeze(0)).view(-1, heads, NTOK, NTOK)
    p = torch.softmax(attn, dim=-1)
    if mutant == "last_key_dropped":
        p = p.clone()
        p[..., NTOK - 1] = 0.0
    vmax = v.abs().amax(dim=-2, keepdim=True).expand(-1, -1, NTOK, -1)

    def unwindow(t):                                          # [Bw][heads][49][32] -> [B][res*res][C] in image order
        t = t.transpose(1, 2).reshape(-1, WS, WS, C)
        t = swin.window_reverse(t, WS, res, res)
        if shift:
            t = torch.roll(t, shifts=(back, back), dims=(1, 2))
        return t.reshape(B, res * res, C)
    ref = unwindow(p @ v)
    tol = TOL * unwindow(vmax) + TOL * ref.abs()
    return ref, tol


def test_cases_cover_every_swin_stage():
    layout = {(res, heads, shift) for (_, _, _, heads, res, shift) in swin.layout()}
    covered = {(res, heads, shift) for (_, res, heads, shift, _) in CASES.values()}
    assert layout <= covered


@pytest.mark.parametrize("name", list(CASES))
def test_mutants_are_far_outside_the_tolerance(name):
    """CPU only: on this case's data each applicable bug moves some output more than MARGIN x its tolerance."""
    qkv, table = make_data(name)
    ref, tol = reference(name, qkv, table)
    if CASES[name][4] == "peaked":
        B, res, heads, _, _ = CASES[name]
        C = HD * heads
        mx = _max_logit(qkv[..., :C].double(), qkv[..., C:2 * C].double(), B, res, heads)
        assert 25.0 < mx < 35.0, mx
    for mut in MUTANTS:
        if not applicable(name, mut):
            continue
        m, _ = reference(name, qkv, table, mut)
        ratio = ((m - ref).abs() / tol).max().item()
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_window_attention_matches_float64(name):
    from imageretrievalresearch_amd._lib import check, lib, stream_ptr
    B, res, heads, shift, _ = CASES[name]
    C = HD * heads
    qkv, table = make_data(name)
    dq, dt = qkv.to(DEV), table.to(DEV).contiguous()
    out = torch.full((B, res * res, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    check(lib().mi355_window_attention(dq.data_ptr(), dt.data_ptr(), out.data_ptr(), B, res, C, heads, shift, stream_ptr(DEV)))
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert torch.isfinite(got).all(), f"{name}: non-finite or unwritten outputs"
    ref, tol = reference(name, qkv, table)
    ratio = (got - ref).abs() / tol
    worst = ratio.max().item()
    print(f"win_attn {name:32s} B={B} res={res} heads={heads} shift={shift}: worst |err| / tol = {worst:.3f}")
    assert worst <= 1.0, f"{name}: worst |err| / tol {worst:.3f} at {np.unravel_index(ratio.argmax().item(), ratio.shape)}"
