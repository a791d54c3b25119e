"""Swin's token kernels (csrc/swin_kernels.hip) on their own, against float64 references: k_layernorm (plain, 2x2 patch-merge
gather, statistics only), k_patch_embed / k_patch_embed96 (fp32, uniform uint8, ragged uint8) and k_ln_token_mean / ..768.

The model-level tests see these kernels through whole-tensor relative L2 at 2e-2, which a gamma read one vector off, a dropped
token or a missing eps passes.  Here every case is one call of a developer entry (mi355_swin_layernorm, mi355_swin_patch_embed,
mi355_swin_ln_token_mean) that goes through the model's launch code, and the comparison is elementwise.

Reference: float64 on the exact bf16 / fp32 / uint8 inputs, timm's formulation (PatchMerging's strided slices and concat, a 4x4
stride-4 convolution as a matrix product over unfolded patches, biased variance with eps inside the square root).  The uint8
modes round to fp32 at SquarePad -> /255 -> (v - mean) / std, where the kernel uses correctly rounded fp32 operations.

Tolerance, elementwise, from the kernels' arithmetic (u = 2^-24; TOL_REL = 2^-8 and TOL_ABS = 2^-20 = 16 u are the project's two
constants, tests/test_gemm_paths_gpu.py):
    bf16 outputs   tol = TOL_REL |ref| + TOL_ABS K (|gamma xhat| + |beta| + |gamma| rstd A)
    (mean, rstd)   tol = TOL_ABS K (A, rstd)
    pooled         tol = TOL_ABS K mean_t(|gamma xhat| + |beta| + |gamma| rstd A)
  * TOL_REL |ref| is the one bf16 rounding of the output.  bf16 keeps 8 significant bits, so that rounding alone is up to
    2^-8 |ref| (1 - 2^-8): a correct kernel with bf16 output reports a worst ratio just under 1, and only the cases with fp32
    output (statistics, pooled) can be expected under 0.5.
  * The second term is fp32 arithmetic.  A is the magnitude the row mean is summed from: mean_c |x_c| for the LayerNorm kernels,
    and for patch-embed a_c + mean_c a_c with a_c = sum_k |x_k w_ck| + |bias_c| (each channel carries its own convolution error
    as well as the row's).  An error of the mean moves every x - mean by the same amount, which rstd amplifies where the row
    mean dwarfs its spread; in the variance it cancels to second order (sum (x - mean) = 0), so rstd has no such term.
  * K is the longest chain of dependent fp32 operations that ends in the reduced value, counted from the code:
      k_layernorm<LPR, VPL>: VPL * 8 in-lane adds, log2(LPR) shuffle adds, one multiply by 1/C       K = 8 VPL + log2 LPR + 1
                             (13 at C = 128 ... 39 at C = 2048; the second pass has the same length)
      k_patch_embed*:        bias + 48 multiply-adds, then LayerNorm over 16 lanes x CPT channels         K = 48 + CPT + 4 + 1
                             (61 at embed 128, 59 at embed 96)
      k_ln_token_mean*:      the LayerNorm chain 16 + 6 + 1 = 23, then ceil(L / 4) adds per wave, 3 adds across the waves and the
                             division by L; the two chains run one after the other, so their lengths add
                                                                                                     K = 23 + ceil(L / 4) + 4
    K is not fitted to GPU output.  Two CPU tests bound the tolerance from both sides: every deliberate bug below lands more than
    MARGIN = 10 tolerances away, and a float32 evaluation of the same formula stays under half of the tolerance on every case.
    For bf16 outputs "half of the tolerance" cannot include the output rounding (see above: that alone is 0.996 of TOL_REL |ref|),
    so there the un-rounded float32 values must stay under half of the fp32 term alone, which asks more of the fp32 arithmetic
    than half of the whole tolerance would, and the values rounded to bf16 must stay inside the whole tolerance.

The `constant` rows (variance exactly 0): the fp32 sum of C equal bf16 values is exact (8 + 11 significant bits), the product
with fl(1/C) is off by at most 2 u |c| (0 when C is a power of two), x - mean is exact, so y - beta is at most
2^-23 * eps^-0.5 |c gamma| = 3.8e-5 |c gamma|.  The case draws |c| <= 2, |gamma| <= 3 and bf16-representable |beta| >= 0.5 (half an
ulp >= 2^-10 = 9.8e-4), so the output must be bf16(beta) bit for bit, and rstd must be eps^-0.5 to fp32 accuracy."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swin_s3_ref
from oracle import swin

DEV = "cuda:0"
TOL_REL, TOL_ABS = 2.0 ** -8, 2.0 ** -20
MARGIN = 10.0
EPS = 1e-5
LN_SHAPE = {96: (4, 3), 192: (8, 3), 384: (16, 3), 768: (32, 3), 1536: (64, 3),      # C -> (LPR, VPL) of launch_ln
            128: (16, 1), 256: (32, 1), 512: (64, 1), 1024: (64, 2), 2048: (64, 4)}
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _tail_rows(C, blocks=2):
    """A few multiples of the rows per block (256 / LPR) plus one: the last block is live in one row only."""
    return blocks * (256 // LN_SHAPE[C][0]) + 1


def _ln(C, kind, *, merge=None, stats=False, rows=None):
    if merge:
        B, gh, gw = merge
        return dict(entry="ln", C=C, kind=kind, merge=1, B=B, gh=gh, gw=gw, stats=0, rows=B * gh * gw)
    return dict(entry="ln", C=C, kind=kind, merge=0, B=1, gh=0, gw=0, stats=int(stats), rows=rows or _tail_rows(C))


def _pe(embed, mode, B, *, H=224, sizes=(), fill=0, b0=0):
    return dict(entry="pe", embed=embed, mode=mode, B=B, H=H, sizes=tuple(sizes), fill=fill, b0=b0)


def _tm(C, L, kind):
    return dict(entry="tm", C=C, B=3, L=L, kind=kind)


RAGGED = ((224, 37), (224, 224), (224, 150), (131, 224), (224, 1))      # descriptor 0 belongs to no launch (b0 = 1)

CASES = {
    # ---- k_layernorm, plain: all ten widths; every data kind on a narrow and on a wide width; the tail row; a single row
    "ln_96_normal": _ln(96, "normal"), "ln_128_normal": _ln(128, "normal"), "ln_192_offset": _ln(192, "offset"),
    "ln_256_near_constant": _ln(256, "near_constant"), "ln_384_constant": _ln(384, "constant"), "ln_512_scaled": _ln(512, "scaled"),
    "ln_768_outlier": _ln(768, "outlier"), "ln_1024_normal": _ln(1024, "normal"), "ln_1536_normal": _ln(1536, "normal"),
    "ln_2048_normal": _ln(2048, "normal"),
    "ln_128_offset": _ln(128, "offset"), "ln_2048_offset": _ln(2048, "offset"),
    "ln_96_near_constant": _ln(96, "near_constant"), "ln_1536_near_constant": _ln(1536, "near_constant"),
    "ln_128_constant": _ln(128, "constant"), "ln_96_constant": _ln(96, "constant"), "ln_2048_constant": _ln(2048, "constant"),
    "ln_1536_constant": _ln(1536, "constant"),
    "ln_96_scaled": _ln(96, "scaled"), "ln_1536_scaled": _ln(1536, "scaled"),
    "ln_128_outlier": _ln(128, "outlier"), "ln_2048_outlier": _ln(2048, "outlier"),
    "ln_1024_one_row": _ln(1024, "normal", rows=1),
    # ---- k_layernorm<MERGE>: gh != gw, two images; the models' own grids; a width no model merges
    "merge_512_3x5": _ln(512, "normal", merge=(2, 3, 5)), "merge_1024_3x5": _ln(1024, "normal", merge=(2, 3, 5)),
    "merge_2048_3x5": _ln(2048, "offset", merge=(2, 3, 5)), "merge_384_3x5": _ln(384, "normal", merge=(2, 3, 5)),
    "merge_768_3x5": _ln(768, "normal", merge=(2, 3, 5)), "merge_1536_3x5": _ln(1536, "normal", merge=(2, 3, 5)),
    "merge_256_3x5": _ln(256, "normal", merge=(2, 3, 5)), "merge_96_5x3": _ln(96, "normal", merge=(3, 5, 3)),
    "merge_1024_7x7": _ln(1024, "normal", merge=(2, 7, 7)), "merge_2048_7x7": _ln(2048, "normal", merge=(1, 7, 7)),
    "merge_1536_7x7": _ln(1536, "normal", merge=(1, 7, 7)), "merge_768_14x14": _ln(768, "normal", merge=(1, 14, 14)),
    "merge_512_28x28": _ln(512, "normal", merge=(1, 28, 28)), "merge_384_28x28": _ln(384, "normal", merge=(1, 28, 28)),
    # ---- k_layernorm<STATS>: the widths the models fold into the next GEMM
    "stats_128_offset": _ln(128, "offset", stats=True), "stats_256_normal": _ln(256, "normal", stats=True),
    "stats_512_near_constant": _ln(512, "near_constant", stats=True), "stats_1024_constant": _ln(1024, "constant", stats=True),
    "stats_192_constant": _ln(192, "constant", stats=True), "stats_384_scaled": _ln(384, "scaled", stats=True),
    "stats_768_offset": _ln(768, "offset", stats=True), "stats_1024_outlier": _ln(1024, "outlier", stats=True),
    "stats_128_far_offset": _ln(128, "far_offset", stats=True), "stats_768_far_offset": _ln(768, "far_offset", stats=True),
    "stats_192_one_row": _ln(192, "normal", stats=True, rows=1),
    # ---- k_patch_embed / k_patch_embed96
    "pe128_f32_h224": _pe(128, "f32", 2), "pe96_f32_h224": _pe(96, "f32", 2),
    "pe128_f32_h12": _pe(128, "f32", 3, H=12), "pe96_f32_h12": _pe(96, "f32", 3, H=12),
    "pe128_f32_h4": _pe(128, "f32", 1, H=4), "pe96_f32_h4": _pe(96, "f32", 1, H=4),
    "pe128_u8_224x224_fill0": _pe(128, "u8", 2, sizes=[(224, 224)], fill=0),
    "pe96_u8_224x224_fill255": _pe(96, "u8", 2, sizes=[(224, 224)], fill=255),
    "pe128_u8_224x150_fill255": _pe(128, "u8", 2, sizes=[(224, 150)], fill=255),
    "pe96_u8_224x150_fill0": _pe(96, "u8", 2, sizes=[(224, 150)], fill=0),
    "pe128_u8_131x224_fill0": _pe(128, "u8", 2, sizes=[(131, 224)], fill=0),
    "pe96_u8_131x224_fill255": _pe(96, "u8", 2, sizes=[(131, 224)], fill=255),
    "pe128_ragged_fill255": _pe(128, "ragged", 4, sizes=RAGGED, fill=255, b0=1),
    "pe96_ragged_fill0": _pe(96, "ragged", 4, sizes=RAGGED, fill=0, b0=1),
    "pe96_ragged_fill255": _pe(96, "ragged", 4, sizes=RAGGED, fill=255, b0=1),
    # ---- k_ln_token_mean / k_ln_token_mean768
    **{f"tm{C}_L{L}_{kind}": _tm(C, L, kind) for C in (1024, 768)
       for L, kind in ((49, "normal"), (1, "normal"), (3, "offset"), (4, "constant"), (50, "offset"), (50, "normal"), (49, "constant"))},
}
LN_CASES = [n for n, c in CASES.items() if c["entry"] == "ln"]
PE_CASES = [n for n, c in CASES.items() if c["entry"] == "pe"]
TM_CASES = [n for n, c in CASES.items() if c["entry"] == "tm"]


def chain_K(c):
    """The K of the module docstring."""
    if c["entry"] == "ln":
        lpr, vpl = LN_SHAPE[c["C"]]
        return 8 * vpl + int(math.log2(lpr)) + 1
    if c["entry"] == "pe":
        return 48 + c["embed"] // 16 + 4 + 1
    return 23 + -(-c["L"] // 4) + 4


# ------------------------------------------------------------------------------------------------------- data (CPU, seeded)
def _bf16(t):
    return t.to(torch.bfloat16)


def _rows_of_kind(kind, R, C, g):
    """[R][C] bf16 rows of one data kind."""
    if kind == "normal":
        x = torch.randn(R, C, generator=g)
    elif kind == "offset":                          # mean around 20, unit spread: a one-pass variance cancels
        x = 20.0 + 0.5 * torch.randn(R, 1, generator=g) + torch.randn(R, C, generator=g)
    elif kind == "far_offset":                      # mean around 200 (bf16 spacing 1 there), spread 2
        x = 200.0 + 5.0 * torch.randn(R, 1, generator=g) + 2.0 * torch.randn(R, C, generator=g)
    elif kind == "near_constant":                   # two neighbouring bf16 values per row: variance (ulp / 2)^2, near eps
        c = _bf16((torch.rand(R, 1, generator=g) * 3.0 + 0.5) * (torch.randint(0, 2, (R, 1), generator=g) * 2 - 1))
        up = (c.view(torch.int16) + 1).view(torch.bfloat16)          # one ulp further from zero
        return torch.where(torch.rand(R, C, generator=g) < 0.5, c.expand(R, C), up.expand(R, C))
    elif kind == "constant":
        c = (torch.rand(R, 1, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (R, 1), generator=g) * 2 - 1)
        x = c.expand(R, C)
    elif kind == "scaled":                          # rows times 2^-10 .. 2^10
        x = torch.randn(R, C, generator=g) * (2.0 ** ((torch.arange(R) % 21) - 10).float()).unsqueeze(1)
    elif kind == "outlier":                         # one element 100 times the rest
        x = torch.randn(R, C, generator=g)
        x[torch.arange(R), torch.randint(0, C, (R,), generator=g)] = 100.0
    else:
        raise KeyError(kind)
    return _bf16(x.contiguous())


def _gamma_beta(kind, C, g):
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    if kind == "constant":                          # see the module docstring: |gamma| <= 3, bf16 beta with |beta| >= 0.5
        gamma = gamma.clamp(-3.0, 3.0)
        beta = _bf16((torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)).float()
    return gamma.contiguous(), beta.contiguous()


_DATA = {}


def make_data(name):
    """The seeded operands of a case (built once, shared by the tests, never modified)."""
    if name in _DATA:
        return _DATA[name]
    c = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    d = {}
    if c["entry"] == "ln":
        # merge: the rows are laid out [B][2 gh][2 gw][C / 4]; the kinds describe the gathered rows closely enough
        R, W = (c["rows"] * 4, c["C"] // 4) if c["merge"] else (c["rows"], c["C"])
        d["x"] = _rows_of_kind(c["kind"], R, W, g)
        d["gamma"], d["beta"] = _gamma_beta(c["kind"], c["C"], g)
    elif c["entry"] == "tm":
        d["x"] = _rows_of_kind(c["kind"], c["B"] * c["L"], c["C"], g).view(c["B"], c["L"], c["C"])
        d["gamma"], d["beta"] = _gamma_beta(c["kind"], c["C"], g)
    else:
        E = c["embed"]
        d["weight"] = (torch.randn(E, 3, 4, 4, generator=g) * 0.2).contiguous()
        d["bias"] = torch.randn(E, generator=g) * 0.1
        d["gamma"], d["beta"] = _gamma_beta("normal", E, g)
        if c["mode"] == "f32":
            d["x"] = torch.randn(c["B"], 3, c["H"], 224, generator=g)
        else:
            sizes = c["sizes"] if c["mode"] == "ragged" else c["sizes"] * c["B"]
            d["images"] = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]
    _DATA[name] = d
    return d


# -------------------------------------------------------------------------------------------------------------- references
MUTANTS = ["eps_left_out", "variance_one_pass_fp32", "gamma_beta_shifted_one_vector", "last_vector_left_out_of_the_mean",
           "merge_parts_swapped", "merge_gh_gw_swapped", "merge_image_index_ignored", "stats_std_for_rstd", "stats_order_swapped",
           "patch_weight_not_transposed", "patch_dy_dx_swapped", "pad_offset_rounded_up", "fill_ignored", "descriptor_b0_ignored",
           "mean_over_L_minus_one", "last_token_dropped", "second_half_of_768_left_out"]


def applicable(name, mutant):
    c = CASES[name]
    e = c["entry"]
    if mutant == "eps_left_out":
        # eps is 1e-5 of a unit variance: only rows whose variance is near or below eps can show it.  (Patch-embed has no such case.)
        return e in ("ln", "tm") and c["kind"] in ("near_constant", "constant")
    if mutant == "variance_one_pass_fp32":
        # fp32 E[x^2] - mean^2 loses 2 log2(mean / spread) bits.  At mean / spread = 20 (`offset`) that is a relative error of rstd
        # of a few hundred u, inside the fp32 tolerance TOL_ABS K = 16 K u and far inside one bf16 rounding: such rows only
        # resolve it where the output is (mean, rstd) and K is smallest, and not by MARGIN.  `far_offset` rows (mean / spread =
        # 100) lose 13 bits, which the statistics output does resolve; the bf16 outputs never see it below mean / spread ~ 1000.
        return e == "ln" and c["stats"] and c["kind"] == "far_offset"
    if mutant in ("gamma_beta_shifted_one_vector", "last_vector_left_out_of_the_mean"):
        # (constant rows: every output is beta, whatever the mean; the statistics kernel reads no gamma)
        if mutant == "gamma_beta_shifted_one_vector":
            return e in ("ln", "tm") and not c.get("stats")
        if e == "tm":                                # (averaged over zero-mean tokens the eight dropped values shrink below the tolerance)
            return c["kind"] == "offset"
        return e == "ln" and c["kind"] != "constant" and c["rows"] > 1          # (one row: eight values may happen to cancel)
    if mutant == "merge_parts_swapped":
        return e == "ln" and c["merge"] == 1
    if mutant == "merge_gh_gw_swapped":
        return e == "ln" and c["merge"] == 1 and c["gh"] != c["gw"]          # gh == gw: the same arithmetic
    if mutant == "merge_image_index_ignored":
        return e == "ln" and c["merge"] == 1 and c["B"] > 1
    if mutant in ("stats_std_for_rstd", "stats_order_swapped"):
        return e == "ln" and c["stats"] == 1
    if mutant in ("patch_weight_not_transposed", "patch_dy_dx_swapped"):
        return e == "pe"
    if mutant == "pad_offset_rounded_up":                                    # (224 - side) odd for some image of the launch
        return e == "pe" and c["mode"] != "f32" and any((224 - h) % 2 or (224 - w) % 2 for h, w in _launched_sizes(c))
    if mutant == "fill_ignored":                                             # a padded image and a fill other than the mutant's 0
        return e == "pe" and c["mode"] != "f32" and c["fill"] != 0 and any(h != w for h, w in _launched_sizes(c))
    if mutant == "descriptor_b0_ignored":
        return e == "pe" and c["mode"] == "ragged" and c["b0"] > 0
    if mutant in ("mean_over_L_minus_one", "last_token_dropped"):
        # (constant rows: every token is beta, so dropping one leaves the mean of L - 1 ... only the divisor shows)
        return e == "tm" and c["L"] > 1 and (mutant == "mean_over_L_minus_one" or c["kind"] != "constant")
    if mutant == "second_half_of_768_left_out":
        return e == "tm" and c["C"] == 768
    raise KeyError(mutant)


def _launched_sizes(c):
    return c["sizes"][c["b0"]:c["b0"] + c["B"]] if c["mode"] == "ragged" else c["sizes"]


def _layernorm64(x, gamma, beta, mutant=None, A=None):
    """LayerNorm over the last dim in float64 -> (y, mean, rstd, tol_second_term / (TOL_ABS K)).  A: see the module docstring."""
    C = x.shape[-1]
    xm = x
    if mutant == "second_half_of_768_left_out":
        xm = x.clone()
        xm[..., 512:] = 0.0
    if mutant == "last_vector_left_out_of_the_mean":
        mean = xm[..., :-8].sum(-1, keepdim=True) / C
    else:
        mean = xm.sum(-1, keepdim=True) / C
    d = x - mean
    if mutant == "variance_one_pass_fp32":
        x32 = x.float()
        var = ((x32 * x32).mean(-1, keepdim=True) - x32.mean(-1, keepdim=True) ** 2).clamp_min(0.0).double()
    elif mutant == "second_half_of_768_left_out":
        var = (d[..., :512] ** 2).sum(-1, keepdim=True) / C
    else:
        var = (d * d).mean(-1, keepdim=True)
    rstd = (var + (0.0 if mutant == "eps_left_out" else EPS)) ** -0.5
    if mutant == "gamma_beta_shifted_one_vector":
        gamma, beta = gamma.roll(-8), beta.roll(-8)
    y = d * rstd * gamma + beta
    if mutant == "second_half_of_768_left_out":
        y[..., 512:] = 0.0
    if A is None:
        A = x.abs().mean(-1, keepdim=True)
    mag = (gamma * d * rstd).abs() + beta.abs() + gamma.abs() * rstd * A
    return y, mean, rstd, mag


def _merge_rows(x, c, mutant=None):
    """[B][2 gh][2 gw][C / 4] -> [B gh gw][C], timm's PatchMerging: x0 = x[:, 0::2, 0::2], x1 = x[:, 1::2, 0::2], x2 = x[:, 0::2, 1::2],
    x3 = x[:, 1::2, 1::2], concatenated.  The index mutants redo the gather from flat offsets with the bug in the arithmetic."""
    B, gh, gw, C4 = c["B"], c["gh"], c["gw"], c["C"] // 4
    if mutant not in ("merge_gh_gw_swapped", "merge_image_index_ignored"):
        v = x.view(B, 2 * gh, 2 * gw, C4)
        parts = [v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]]
        if mutant == "merge_parts_swapped":
            parts[1], parts[2] = parts[2], parts[1]
        return torch.cat(parts, -1).reshape(B * gh * gw, 4 * C4)
    if mutant == "merge_gh_gw_swapped":
        gh, gw = gw, gh
    r = torch.arange(c["rows"]).view(-1, 1)
    part = torch.arange(4).view(1, -1)
    bimg = r // (gh * gw)
    rem = r - bimg * gh * gw
    oy, ox = rem // gw, rem % gw
    if mutant == "merge_image_index_ignored":
        bimg = bimg * 0
    src = (bimg * (2 * gh) + 2 * oy + (part & 1)) * (2 * gw) + 2 * ox + (part >> 1)          # [rows][4] source token
    return x.view(-1, C4)[src.reshape(-1)].reshape(c["rows"], 4 * C4)


def _square_pad_normalize(img, fill, round_up=False):
    """uint8 [h][w][3] -> float64 [3][224][224]: SquarePad(fill) -> /255 -> (v - mean) / std, each of the three in fp32."""
    h, w, _ = img.shape
    vp, hp = ((224 - h + 1) // 2, (224 - w + 1) // 2) if round_up else ((224 - h) // 2, (224 - w) // 2)
    canvas = np.full((224, 224, 3), fill, np.uint8)
    canvas[vp:vp + h, hp:hp + w] = img.numpy()
    v = canvas.astype(np.float32) / np.float32(255.0)
    v = (v - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)
    assert v.dtype == np.float32
    return torch.from_numpy(v).permute(2, 0, 1).double()


def _patch_input(name, mutant=None):
    c, d = CASES[name], make_data(name)
    if c["mode"] == "f32":
        return d["x"].double()
    first = 0 if mutant == "descriptor_b0_ignored" else c["b0"]
    imgs = d["images"][first:first + c["B"]]
    fill = 0 if mutant == "fill_ignored" else c["fill"]
    return torch.stack([_square_pad_normalize(i, fill, mutant == "pad_offset_rounded_up") for i in imgs])


def reference(name, mutant=None):
    """(ref, tol) float64, elementwise, in the layout of the entry's output.  `mutant` names a deliberate bug."""
    c, d = CASES[name], make_data(name)
    K = chain_K(c)
    gamma, beta = d["gamma"].double(), d["beta"].double()
    if c["entry"] == "ln":
        x = d["x"].double()
        rows = _merge_rows(x, c, mutant) if c["merge"] else x
        y, mean, rstd, mag = _layernorm64(rows, gamma, beta, mutant)
        if not c["stats"]:
            return y, TOL_REL * y.abs() + TOL_ABS * K * mag
        st = torch.cat([mean, rstd], 1)
        if mutant == "stats_std_for_rstd":
            st = torch.cat([mean, 1.0 / rstd], 1)
        elif mutant == "stats_order_swapped":
            st = torch.cat([rstd, mean], 1)
        return st, TOL_ABS * K * torch.cat([rows.abs().mean(-1, keepdim=True), rstd], 1)
    if c["entry"] == "tm":
        y, _, _, mag = _layernorm64(d["x"].double(), gamma, beta, mutant)
        L = c["L"]
        if mutant == "last_token_dropped":
            y = y[:, :L - 1]
        pooled = y.sum(1) / (L - 1 if mutant == "mean_over_L_minus_one" else L)
        return pooled, TOL_ABS * K * mag.mean(1)
    X = _patch_input(name, mutant)                                            # [B][3][H][224]
    B, E, gh = c["B"], c["embed"], c["H"] // 4
    p = X.view(B, 3, gh, 4, 56, 4).permute(0, 2, 4, 1, 3, 5)                  # [B][py][px][ci][dy][dx]
    if mutant == "patch_dy_dx_swapped":
        p = p.transpose(-1, -2)
    p = p.reshape(B, gh * 56, 48)
    W = _bf16(d["weight"]).double().view(E, 48)                              # the model packs bf16-rounded weights
    if mutant == "patch_weight_not_transposed":
        W = W.reshape(48, E).t()                                              # [co][k] read where [k][co] belongs
    conv = p @ W.t() + d["bias"].double()
    a = p.abs() @ W.abs().t() + d["bias"].double().abs()
    y, _, _, mag = _layernorm64(conv, gamma, beta, mutant, A=a + a.mean(-1, keepdim=True))
    return y, TOL_REL * y.abs() + TOL_ABS * K * mag


def float32_evaluation(name):
    """The same formula in float32 (torch, CPU), before the output rounding -> (values, output is bf16)."""
    c, d = CASES[name], make_data(name)
    if c["entry"] == "ln":
        x = d["x"].float()
        rows = _merge_rows(x, c) if c["merge"] else x
        if c["stats"]:
            mean = rows.mean(-1, keepdim=True)
            return torch.cat([mean, torch.rsqrt(rows.var(-1, unbiased=False, keepdim=True) + EPS)], 1), False
        return F.layer_norm(rows, (c["C"],), d["gamma"], d["beta"], EPS), True
    if c["entry"] == "tm":
        return F.layer_norm(d["x"].float(), (c["C"],), d["gamma"], d["beta"], EPS).mean(1), False
    X = _patch_input(name).float()
    B, E, gh = c["B"], c["embed"], c["H"] // 4
    p = X.view(B, 3, gh, 4, 56, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * 56, 48)
    conv = p @ _bf16(d["weight"]).float().view(E, 48).t() + d["bias"]
    return F.layer_norm(conv, (E,), d["gamma"], d["beta"], EPS), True


def _ratio(got, ref, tol):
    """|got - ref| / tol, elementwise; a non-finite output counts as infinitely far."""
    r = (got - ref).abs() / tol
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))


# --------------------------------------------------------------------------------------------------------------- CPU tests
def test_cases_cover_every_layernorm_of_both_models():
    ln = [CASES[n] for n in LN_CASES]
    covered = {(c["C"], c["merge"]) for c in ln if not c["stats"]}
    merged = {(c["C"], c["gh"], c["gw"]) for c in ln if c["merge"]}
    stats = {c["C"] for c in ln if c["stats"]}
    for embed, depths, img, patch in ((swin.EMBED, swin.DEPTHS, swin.IMG, swin.PATCH),
                                      (swin_s3_ref.EMBED, swin_s3_ref.DEPTHS, swin_s3_ref.IMG, swin_s3_ref.PATCH)):
        for s in range(len(depths)):
            dim, res = embed * 2 ** s, img // patch // 2 ** s
            assert (dim, 0) in covered, dim
            if dim >= 128 and dim % 64 == 0:                 # swin_exec folds these widths into the next GEMM (rows >= 1024)
                assert dim in stats, dim
            if s + 1 < len(depths):                          # PatchMerging to the next stage: LayerNorm(4 dim) on a res/2 grid
                assert (4 * dim, 1) in covered, dim
                assert (4 * dim, res // 2, res // 2) in merged or (4 * dim, 7, 7) in merged, (dim, res)
        assert any(CASES[n]["C"] == embed * 2 ** (len(depths) - 1) for n in TM_CASES)
    assert {CASES[n]["embed"] for n in PE_CASES} == {swin.EMBED, swin_s3_ref.EMBED}
    assert {c["C"] for c in ln if not c["merge"] and not c["stats"]} == set(LN_SHAPE)          # all ten widths, plain
    assert {c["C"] for c in ln if c["merge"]} >= {512, 1024, 2048, 384, 768, 1536}
    assert any(c["merge"] and c["gh"] != c["gw"] for c in ln) and any(c["rows"] == 1 for c in ln)
    for kind in ("normal", "offset", "near_constant", "constant", "scaled", "outlier"):
        widths = {c["C"] for c in ln if c["kind"] == kind and not c["merge"]}
        assert min(widths) <= 128 and max(widths) >= 1536, kind
    for n in LN_CASES:                                        # the row tail is live: the last block holds fewer rows than it could
        c = CASES[n]                                          # (the models' own square grids fill their blocks exactly)
        assert (c["merge"] and c["gh"] == c["gw"]) or c["rows"] % (256 // LN_SHAPE[c["C"]][0]) != 0, n
    assert {(CASES[n]["C"], CASES[n]["L"]) for n in TM_CASES} >= {(C, L) for C in (1024, 768) for L in (49, 1, 3, 4, 50)}


def test_every_mutant_applies_somewhere():
    for mut in MUTANTS:
        assert any(applicable(n, mut) for n in CASES), mut


@pytest.mark.parametrize("name", [n for n in LN_CASES + TM_CASES if CASES[n]["kind"] in ("near_constant", "constant", "offset")])
def test_data_kinds_are_what_they_claim(name):
    c, d = CASES[name], make_data(name)
    x = d["x"].double().reshape(-1, d["x"].shape[-1])
    var = x.var(-1, unbiased=False)
    if c["kind"] == "near_constant":                          # eps decides the answer: variance within a decade of it
        assert (var > EPS / 10).all() and (var < EPS * 10).all(), (var.min().item(), var.max().item())
        assert all(len(r.unique()) == 2 for r in x)
    elif c["kind"] == "constant":
        assert (var == 0).all()
        assert (d["beta"] == _bf16(d["beta"]).float()).all() and d["beta"].abs().min() >= 0.5
        assert x.abs().max() <= 2.0 and d["gamma"].abs().max() <= 3.0
    else:
        assert (x.mean(-1).abs() > 15).all() and (var.sqrt() < 2.5).all()


@pytest.mark.parametrize("name", list(CASES))
def test_float32_evaluation_stays_under_half_the_tolerance(name):
    """The tolerance is not tighter than fp32 arithmetic and one bf16 rounding allow (module docstring, on K)."""
    ref, tol = reference(name)
    assert torch.isfinite(ref).all() and (tol > 0).all()
    y32, rounds = float32_evaluation(name)
    fp32_term = tol - TOL_REL * ref.abs() if rounds else tol
    worst = _ratio(y32.double(), ref, fp32_term).max().item()
    assert worst <= 0.5, f"{name}: float32 evaluation at {worst:.3f} of the fp32 term of the tolerance"
    if rounds:
        worst = _ratio(_bf16(y32).double(), ref, tol).max().item()
        assert worst <= 1.0, f"{name}: float32 evaluation rounded to bf16 at {worst:.3f} of the tolerance"


@pytest.mark.parametrize("name", [n for n in CASES if any(applicable(n, m) for m in MUTANTS)])
def test_mutants_are_far_outside_the_tolerance(name):
    """CPU only: on this case's data each applicable bug moves some output more than MARGIN x its tolerance."""
    ref, tol = reference(name)
    for mut in MUTANTS:
        if not applicable(name, mut):
            continue
        m, _ = reference(name, mut)
        ratio = _ratio(m, ref, tol).max().item()
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


# --------------------------------------------------------------------------------------------------------------------- GPU
def _report(what, name, got, ref, tol):
    assert torch.isfinite(got).all(), f"{name}: non-finite or unwritten outputs"
    ratio = (got - ref).abs() / tol
    worst = ratio.max().item()
    print(f"{what} {name:28s}: worst |err| / tol = {worst:.3f}")
    assert worst <= 1.0, f"{name}: worst |err| / tol {worst:.3f} at {np.unravel_index(ratio.argmax().item(), ratio.shape)}"


def _layernorm_on_gpu(x, gamma, beta, rows, C, merge=0, gh=0, gw=0, stats=0):
    from imageretrievalresearch_amd._lib import check, lib, stream_ptr
    dx = x.to(DEV).contiguous()
    dg, db = gamma.to(DEV), beta.to(DEV)
    out = torch.full((rows, 2) if stats else (rows, C), float("nan"), device=DEV, dtype=torch.float32 if stats else torch.bfloat16)
    check(lib().mi355_swin_layernorm(dx.data_ptr(), None if stats else dg.data_ptr(), None if stats else db.data_ptr(), out.data_ptr(),
                                     rows, C, merge, gh, gw, stats, EPS, stream_ptr(DEV)))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", LN_CASES)
def test_layernorm_matches_float64(name):
    c, d = CASES[name], make_data(name)
    out = _layernorm_on_gpu(d["x"], d["gamma"], d["beta"], c["rows"], c["C"], c["merge"], c["gh"], c["gw"], c["stats"]).cpu()
    ref, tol = reference(name)
    _report("layernorm", name, out.double(), ref, tol)
    if c["kind"] == "constant" and c["stats"]:
        assert ((out[:, 1].double() * math.sqrt(EPS) - 1.0).abs() <= TOL_ABS).all(), f"{name}: rstd is not eps^-0.5"
    elif c["kind"] == "constant":
        want = _bf16(d["beta"]).expand(c["rows"], c["C"])
        assert torch.equal(out.view(torch.int16), want.contiguous().view(torch.int16)), f"{name}: constant rows must give bf16(beta)"


@pytest.mark.gpu
@pytest.mark.parametrize("name", PE_CASES)
def test_patch_embed_matches_float64(name):
    import ctypes

    from imageretrievalresearch_amd._lib import check, lib, stream_ptr
    c, d = CASES[name], make_data(name)
    B, E, L = c["B"], c["embed"], (c["H"] // 4) * 56
    w, bias, gamma, beta = (d[k].to(DEV).contiguous() for k in ("weight", "bias", "gamma", "beta"))
    out = torch.full((B, L, E), float("nan"), device=DEV, dtype=torch.bfloat16)
    x = images = desc = mean = stdv = None
    h = wd = 0
    if c["mode"] == "f32":
        x = d["x"].to(DEV).contiguous()
    else:
        images = torch.cat([i.reshape(-1) for i in d["images"]]).to(DEV)
        mean, stdv = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
        if c["mode"] == "ragged":
            off = np.cumsum([0] + [i.numel() for i in d["images"]])[:-1]
            desc = torch.tensor([[int(o), i.shape[0], i.shape[1]] for o, i in zip(off, d["images"])], dtype=torch.int64).to(DEV)
        else:
            h, wd = c["sizes"][0]
    check(lib().mi355_swin_patch_embed(None if x is None else x.data_ptr(), None if images is None else images.data_ptr(),
                                       None if desc is None else desc.data_ptr(), c["b0"], B, c["H"], h, wd, c["fill"], mean, stdv,
                                       w.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), E, EPS, out.data_ptr(),
                                       stream_ptr(DEV)))
    torch.cuda.synchronize()
    ref, tol = reference(name)
    _report("patch_embed", name, out.cpu().double(), ref, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TM_CASES)
def test_ln_token_mean_matches_float64(name):
    from imageretrievalresearch_amd._lib import check, lib, stream_ptr
    c, d = CASES[name], make_data(name)
    x, gamma, beta = d["x"].to(DEV).contiguous(), d["gamma"].to(DEV), d["beta"].to(DEV)
    pooled = torch.full((c["B"], c["C"]), float("nan"), device=DEV)
    pooled_bf16 = torch.full((c["B"], c["C"]), float("nan"), device=DEV, dtype=torch.bfloat16)
    check(lib().mi355_swin_ln_token_mean(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), pooled.data_ptr(), pooled_bf16.data_ptr(),
                                         c["B"], c["L"], c["C"], EPS, stream_ptr(DEV)))
    torch.cuda.synchronize()
    ref, tol = reference(name)
    _report("ln_token_mean", name, pooled.cpu().double(), ref, tol)
    assert torch.equal(pooled_bf16.cpu().view(torch.int16), _bf16(pooled.cpu()).view(torch.int16)), f"{name}: pooled_bf16 != bf16(pooled)"


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", [(256, 384), (192, 576)])
def test_stats_feed_the_folded_gemm(K, N):
    """(mean, rstd) as k_layernorm<STATS> writes them are what the GEMM's LayerNorm-folded epilogue reads: LayerNorm -> Linear
    through mi355_swin_layernorm(stats = 1) + mi355_gemm_bf16_ex against float64, under test_gemm_paths_gpu.py's tolerance."""
    import ctypes

    from imageretrievalresearch_amd._lib import GemmExArgs, check, lib, stream_ptr
    M = 1100
    g = torch.Generator().manual_seed(K + N)
    x = _bf16(0.7 + 0.3 * torch.randn(M, 1, generator=g) + torch.randn(M, K, generator=g) * (0.5 + torch.rand(M, 1, generator=g)))
    gamma = ((torch.rand(K, generator=g) + 0.5) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1)).double()
    beta = torch.randn(K, generator=g).double()
    Wf = _bf16(torch.randn(N, K, generator=g) / math.sqrt(K))                  # the folded weights W' = W gamma, as packed
    W = Wf.double() / gamma                                                  # the Linear they came from
    bias = (torch.randn(N, generator=g) * 0.1).double()
    bias_f = (bias + W @ beta).float()                                       # b' = b + W beta
    colsum = Wf.double().sum(1).float()
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    rstd = ((xd - mean).pow(2).mean(-1, keepdim=True) + EPS) ** -0.5
    ref = ((xd - mean) * rstd * gamma + beta) @ W.t() + bias
    mag = rstd * (xd.abs() @ Wf.double().abs().t() + (mean * colsum.double()).abs())
    tol = TOL_REL * ref.abs() + TOL_ABS * mag
    dx = x.to(DEV).contiguous()
    stats = torch.full((M, 2), float("nan"), device=DEV)
    check(lib().mi355_swin_layernorm(dx.data_ptr(), None, None, stats.data_ptr(), M, K, 0, 0, 0, 1, EPS, stream_ptr(DEV)))
    dW, db, dc = Wf.to(DEV).contiguous(), bias_f.to(DEV), colsum.to(DEV)
    out = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    a = GemmExArgs(A=dx.data_ptr(), lda=K, W=dW.data_ptr(), ldw=K, bias=db.data_ptr(), out=out.data_ptr(), ldo=N, M=M, N=N, K=K,
                   ln_stats=stats.data_ptr(), ln_colsum=dc.data_ptr())
    path = ctypes.c_int(-1)
    check(lib().mi355_gemm_bf16_ex(ctypes.byref(a), ctypes.byref(path), stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert path.value & 0xff == 4, f"the folded epilogue belongs to the DMA-tiled kernel (path {path.value})"
    _report("ln -> gemm", f"chain_K{K}_N{N}", out.cpu().double(), ref, tol)
