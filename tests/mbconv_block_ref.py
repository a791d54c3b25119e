"""Float64 reference, tolerances, launcher rules and cases for the whole-block MBConv kernel (k_mbconv_block, csrc/mbconv_block.hip),
reached through the developer entry mi355_mbconv_block_ex.  Plain torch / numpy on the CPU; tests/test_mbconv_block_gpu.py holds
the tests.

Rounding points of the kernel:
    E  = bf16(act_e(fp32 MFMA sum + be))                 lives only in the LDS
    D  = bf16(act_d(fp32 MFMA tap sum + bd))             the kernel's scratch, read back by the test
    squeeze = (sum of the un-rounded fp32 act_d values) * inv_hw, inv_hw = 1 / (Ho Wo)
    FC1, FC2 and the sigmoid in fp32 on bf16 weights     gate g, never rounded to bf16
    A' = bf16(relu6?(D g))                               fp32 product of the ROUNDED D and the gate
    Y  = bf16(fp32 MFMA sum + bp + X[..., n] for n < res_n)

The comparison is staged, so that a rounding that fell the other way upstream does not loosen the check downstream.

D: the rule of tests/mbconv_front_ref.py, imported: e_r rounded from float64, one ulp of slack for the flippable E elements,
    |D - d64| <= 2^-8 |d64| + deriv_d (2^-18 magD + sum_taps |wd| slack)                               TOL_REL, TOL_DW, TOL_E

Y: from the kernel's own D (D_k: exact bf16 values), so nothing of D's error is carried.  The squeeze s64 is the mean of the
un-rounded float64 depthwise values, and ds the squeeze bound of mbconv_front_ref.  The gate follows test_conv_paths_gpu.py:
    r64 = se_act(s64 W1^T + b1)       g64 = sigmoid(r64 W2 + b2)
    mag_s = ds / 2^-18                mag_r = deriv_se (mag_s |W1|^T + |b1|)        mag_g = 0.25 (mag_r |W2| + |b2|)
    dg = 2^-18 (mag_g + |g64|)                                                                         TOL_SE, DERIV
(in test_conv_paths_gpu.py the squeeze bound IS 2^-18 mag_s; here it is ds, which also holds the slack of the flippable E
elements, and it goes through both FCs by the same worst-case sums).
    a64 = relu6?(D_k g64)             a_r = round_bf16(a64) on the float64 value
    an A' element is flippable when midpoint_distance(a64) <= |D_k| dg + 2^-23 |a64| (the gate's error, and the fp32 product);
    it then has slack_a = one bf16 ulp
    y64 = sum_k a_r Wp + bp + res     magY = sum_k |a_r| |Wp| + |bp| + |res|
    |Y - y64| <= 2^-8 |y64| + 2^-20 magY + sum_k slack_a |Wp|
2^-8 is the one bf16 rounding of Y, 2^-20 the fp32-accumulation coefficient of test_gemm_paths_gpu.py (a STATISTICAL bound: a
correct kernel that exceeded it would call for the worst-case n 2^-24 term, not a looser coefficient).  Every coefficient is one
the suite already uses.  The flippable shares of a case's E elements and of its A' elements must each stay at or below FLIP_CAP;
the data is scaled for that: the SE weights of a column share their sign, so that the worst-case sums behind mag_g stay near the
values themselves (random signs would make mag_g ~ sqrt(rd mid) times the gate's spread and every A' element flippable)."""
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

from imageretrievalresearch_amd import synth
from mbconv_front_ref import (ACT_NONE, ACT_RELU, ACT_SILU, DERIV, FLIP_CAP, GUARD, MARGIN, TOL_E, TOL_REL, _act, cdiv, kpad32,
                              midpoint_distance, round_bf16, ulp_bf16)
from mbconv_front_ref import Case as FrontCase
from mbconv_front_ref import reference as front_reference

TOL_SE = 2.0 ** -18         # tests/test_conv_paths_gpu.py
TOL_ACC = TOL_E             # 2^-20: the fp32-accumulation coefficient of tests/test_gemm_paths_gpu.py
TOL_MUL = 2.0 ** -23        # one fp32 rounding (the product D g)
ROT_B = 11                  # batch of the batch-position test: more images than any rotation period of its cases

# ------------------------------------------------------------------------------------- the launcher's rules, written out
MB_THREADS, MB_WAVES, MB_MAX_RD, MB_MC, LDS_MAX = 512, 8, 192, 128, 160 * 1024
# (depthwise k, stride, map width, expand k-steps, projection column tiles per wave, depthwise activation): MB_INSTANCES
INSTANCES = [(3, 1, 14, 3, 3, ACT_SILU), (5, 1, 14, 3, 3, ACT_SILU), (5, 1, 14, 5, 3, ACT_SILU), (5, 2, 14, 5, 2, ACT_SILU),
             (5, 1, 7, 8, 2, ACT_SILU), (3, 1, 7, 8, 3, ACT_SILU), (3, 1, 7, 12, 3, ACT_SILU),
             (3, 1, 14, 4, 2, ACT_NONE), (3, 1, 14, 4, 3, ACT_NONE), (3, 1, 14, 5, 3, ACT_NONE), (3, 1, 14, 6, 3, ACT_NONE),
             (3, 1, 7, 7, 2, ACT_NONE), (3, 1, 7, 8, 2, ACT_NONE), (3, 1, 7, 8, 3, ACT_NONE), (3, 1, 7, 9, 3, ACT_NONE),
             (3, 1, 7, 10, 3, ACT_NONE), (3, 1, 7, 11, 3, ACT_NONE), (3, 1, 14, 6, 4, ACT_NONE)]


def block_path(ks, s, wi, kst, ntw, act_d, xwide, whole, nsc, js):
    """MI355_BLOCK_PATH of include/mi355_retrieval.h"""
    return (int(ks == 5) | int(s == 2) << 1 | int(wi == 14) << 2 | kst << 3 | ntw << 7 | act_d << 10 | int(bool(xwide)) << 13 |
            int(bool(whole)) << 14 | nsc << 15 | js << 20)


def path_fields(p):
    """the MI355_BLOCK_PATH_* accessors"""
    return dict(ks=5 if p & 1 else 3, s=2 if p >> 1 & 1 else 1, wi=14 if p >> 2 & 1 else 7, kst=p >> 3 & 15, ntw=p >> 7 & 7,
                act_d=p >> 10 & 7, xwide=p >> 13 & 1, whole=p >> 14 & 1, nsc=p >> 15 & 31, js=p >> 20 & 15)


def conv_out(h, k, s):
    return (h + 2 * (k // 2) - k) // s + 1


def mb_geom(H, W):
    """(wi, mw, mh, ntw, mwp, a_it) or None"""
    if W == 7 and H * W <= 64:
        return (7, 4, 1, 3, 4, 4)
    if W == 14 and H * W <= 208:
        return (14, 7, 2, 3, 7, 7)
    return None


def mb_proj_ntw(NTp, MTp, NTW):
    best, best_busy = 1, 0
    for ntw in range(1, NTW + 1):
        nwn = cdiv(NTp, ntw)
        if nwn > MB_WAVES:
            continue
        busy = nwn * min(MB_WAVES // nwn, MTp)
        if busy >= best_busy:
            best_busy, best = busy, ntw
    return best


def mb_pick_ntw(NTp, MTp, wi, mwp):
    ntw = mb_proj_ntw(NTp, MTp, 3)
    if wi != 14:
        return ntw
    nwn = cdiv(NTp, ntw)
    msplit = min(MB_WAVES // nwn if nwn <= MB_WAVES else 1, MTp)
    if nwn <= MB_WAVES and cdiv(MTp, msplit) <= mwp:
        return ntw
    return 4


def mb_instance_ok(k, stride, wi, kst, ntw, act_d):
    return (k, stride, wi, kst, ntw, act_d) in INSTANCES


def mb_fc2_slices(mid):
    return max(1, min(8, MB_THREADS // (mid // 8)))


def mb_pick_kcs(W, Pout, mid):
    q = 256 if W == 7 else 128
    avail = LDS_MAX - ((mid + 255) & ~255) * 4
    kmax = (avail // Pout // 2 - 16) // q * q
    if kmax < q:
        return 0
    Kp2 = kpad32(mid)
    nsc = cdiv(Kp2, kmax)
    return cdiv(cdiv(Kp2, nsc), q) * q


def mb_lds_bytes_xld(H, W, Ho, Wo, mid, Cout, k, xld, wi):
    """LDS bytes for an X row stride of xld elements; 0 = does not fit"""
    P, pad = H * W, k // 2
    MT, ew = cdiv(P, 16), W + 2 * pad
    stride = 2 if (H + 2 * pad - k) // (Ho - 1 if Ho > 1 else 1) >= 2 else 1
    rp = (ew + 7) & ~7 if (Wo <= 8 and stride == 1) else ew
    EP = (H + 2 * pad + (stride if Wo <= 8 else 0)) * rp + 8
    xs, pl = (MT * 16 * xld * 2 + 64 + 15) & ~15, ((mid + 255) & ~255) * 4
    fixed = xs + pl + MB_MAX_RD * 4
    slab = MB_WAVES * EP * 16 * 2
    Pout = Ho * Wo
    se = mb_fc2_slices(mid) * mid * 4
    kcs = mb_pick_kcs(W, Pout, mid)
    if not kcs:
        return 0
    kc, MTp = 256 if wi == 7 else 128, cdiv(Pout, 16)
    whole = wi == 7 and mb_proj_ntw(cdiv(Cout, 16), MTp, 3) == 2
    proj = pl + (Pout * (kcs + 16) * 2 if whole else 2 * MTp * 16 * (kc + 16) * 2)
    total = max(fixed + max(slab, se), proj)
    return total if total <= LDS_MAX else 0


def mb_pick_xld(H, W, Ho, Wo, Cin, mid, Cout, k, wi):
    wide, compact = kpad32(Cin) + 16, ((Cin + 7) & ~7) + 8
    if mb_lds_bytes_xld(H, W, Ho, Wo, mid, Cout, k, wide, wi):
        return wide
    if mb_lds_bytes_xld(H, W, Ho, Wo, mid, Cout, k, compact, wi):
        return compact
    return 0


def mbconv_block_supported(H, W, Cin, mid, Cout, k, stride, rd, act_e, act_d):
    g = mb_geom(H, W)
    if g is None or act_e != ACT_SILU:
        return False
    wi, mw, mh, _, mwp, a_it = g
    if Cin % 8 or mid % 8 or mid > 2560 or Cout % 8 or rd < 1 or rd > MB_MAX_RD:
        return False
    if k not in (3, 5) or stride not in (1, 2) or (W == 7 and stride == 2):
        return False
    if mid * kpad32(Cin) >= 1 << 30 or Cout * mid >= 1 << 30:
        return False
    Ho, Wo = conv_out(H, k, stride), conv_out(W, k, stride)
    Pout = Ho * Wo
    MTp, NTp = cdiv(Pout, 16), cdiv(Cout, 16)
    ntw = mb_pick_ntw(NTp, MTp, wi, mwp)
    nwn = cdiv(NTp, ntw)
    if nwn > MB_WAVES:
        return False
    if cdiv(MTp, min(MB_WAVES // nwn, MTp)) > mwp:
        return False
    if Pout * (32 if wi == 7 else 16) > a_it * MB_THREADS:
        return False
    if cdiv(H * W, 16) > mw * mh:
        return False
    if not mb_instance_ok(k, stride, wi, kpad32(Cin) // 32, ntw, act_d):
        return False
    return mb_pick_xld(H, W, Ho, Wo, Cin, mid, Cout, k, wi) != 0


def block_how(H, W, Cin, mid, Cout, k, stride, rd, act_e, act_d):
    """what mi355_mbconv_block_how reports: the path, or None for a shape the kernel does not take"""
    if not mbconv_block_supported(H, W, Cin, mid, Cout, k, stride, rd, act_e, act_d):
        return None
    wi, _, _, _, mwp, _ = mb_geom(H, W)
    Ho, Wo = conv_out(H, k, stride), conv_out(W, k, stride)
    ntw = mb_pick_ntw(cdiv(Cout, 16), cdiv(Ho * Wo, 16), wi, mwp)
    xld = mb_pick_xld(H, W, Ho, Wo, Cin, mid, Cout, k, wi)
    kcs = mb_pick_kcs(W, Ho * Wo, mid)
    return block_path(k, stride, wi, kpad32(Cin) // 32, ntw, act_d, xld == kpad32(Cin) + 16, wi == 7 and ntw == 2,
                      cdiv(kpad32(mid), kcs), mb_fc2_slices(mid))


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    H: int
    W: int
    Cin: int
    mid: int
    Cout: int
    k: int
    stride: int
    rd: int
    act_d: int = ACT_SILU
    se_act: int = ACT_SILU
    a_relu6: int = 0
    res_n: int = 0              # 0: no residual
    B: int = 3
    model: str = ""             # the model whose 224 x 224 plan runs this block shape
    same: bool = False          # every image is image 0 (the batch-position test)
    seed: int = 0

    @property
    def Ho(self):
        return conv_out(self.H, self.k, self.stride)

    @property
    def Wo(self):
        return conv_out(self.W, self.k, self.stride)

    @property
    def Pout(self):
        return self.Ho * self.Wo

    @property
    def shape(self):
        return (self.H, self.W, self.Cin, self.mid, self.Cout, self.k, self.stride, self.rd, ACT_SILU, self.act_d)

    @property
    def supported(self):
        return mbconv_block_supported(*self.shape)

    @property
    def code(self):
        """the `path` the entry must report"""
        return block_how(*self.shape)

    @property
    def f(self):
        return path_fields(self.code)

    @property
    def instance(self):
        f = self.f
        return (f["ks"], f["s"], f["wi"], f["kst"], f["ntw"], f["act_d"])

    @property
    def square(self):
        return self.H == self.W

    @property
    def nslabs(self):
        return cdiv(self.mid, MB_MC)

    @property
    def ngroups(self):
        """FC1 groups of four hidden units"""
        return cdiv(self.rd, 4)

    @property
    def nwn(self):
        """waves along N in the projection: the period of the column-group rotation"""
        return cdiv(cdiv(self.Cout, 16), self.f["ntw"])

    @property
    def nchunks(self):
        """K chunks of the double-buffered projection flavour"""
        return cdiv(kpad32(self.mid), 256 if self.W == 7 else 128)

    @property
    def counted_wait(self):
        """the slab loop takes the counted s_waitcnt (MTo == MTO_SQ) and not vmcnt(0)"""
        two = self.Wo <= 8
        mto = (self.Ho + 1) // 2 if two else self.Ho
        return mto == ((self.Wo + 1) // 2 if two else self.Wo)

    @property
    def front(self):
        """the same expand + depthwise pair as a case of mbconv_front_ref (its reference needs no more than the shape)"""
        return FrontCase("late", self.B, self.H, self.W, self.Cin, self.mid, self.k, self.stride, act_e=ACT_SILU, act_d=self.act_d)


SILU = dict(act_d=ACT_SILU, se_act=ACT_SILU, a_relu6=0)          # efficientnet_b3a
LIN = dict(act_d=ACT_NONE, se_act=ACT_RELU, a_relu6=1)           # rexnet: linear depthwise, ReLU in the SE, ReLU6 behind the gate


def pad8(c):
    return (c + 7) & ~7


# every block shape the three models' plans run whole-block at 224 x 224 (the launch plan golden's "block" steps at B = 256):
# (model, map, Cin, mid, Cout, k, stride, rd, residual), channel counts as the models have them (the packer pads them to 8)
MODEL_LAYERS = [
    ("efficientnet_b3a", 14, 96, 576, 96, 3, 1, 24, True), ("efficientnet_b3a", 14, 96, 576, 136, 5, 1, 24, False),
    ("efficientnet_b3a", 14, 136, 816, 136, 5, 1, 34, True), ("efficientnet_b3a", 14, 136, 816, 232, 5, 2, 34, False),
    ("efficientnet_b3a", 7, 232, 1392, 232, 5, 1, 58, True), ("efficientnet_b3a", 7, 232, 1392, 384, 3, 1, 58, False),
    ("efficientnet_b3a", 7, 384, 2304, 384, 3, 1, 96, True),
    ("rexnet_150", 14, 108, 648, 125, 3, 1, 54, True), ("rexnet_150", 14, 125, 750, 142, 3, 1, 62, True),
    ("rexnet_150", 14, 142, 852, 159, 3, 1, 71, True), ("rexnet_150", 14, 159, 954, 176, 3, 1, 79, True),
    ("rexnet_150", 14, 176, 1056, 193, 3, 1, 88, True), ("rexnet_150", 7, 210, 1260, 226, 3, 1, 105, True),
    ("rexnet_150", 7, 226, 1356, 243, 3, 1, 113, True), ("rexnet_150", 7, 243, 1458, 260, 3, 1, 121, True),
    ("rexnet_150", 7, 260, 1560, 277, 3, 1, 130, True),
    ("rexnet_200", 14, 144, 864, 167, 3, 1, 72, True), ("rexnet_200", 14, 167, 1002, 190, 3, 1, 83, True),
    ("rexnet_200", 14, 190, 1140, 212, 3, 1, 95, True), ("rexnet_200", 7, 280, 1680, 302, 3, 1, 140, True),
    ("rexnet_200", 7, 302, 1812, 324, 3, 1, 151, True), ("rexnet_200", 7, 324, 1944, 347, 3, 1, 162, True),
    ("rexnet_200", 7, 347, 2082, 370, 3, 1, 173, True)]


def model_case(model, m, cin, mid, cout, k, s, rd, res):
    eff = model.startswith("eff")
    # efficientnet: the shortcut covers every output channel; rexnet: the block's (padded) input channels
    res_n = 0 if not res else (pad8(cout) if eff else pad8(cin))
    return Case(m, m, pad8(cin), pad8(mid), pad8(cout), k, s, rd, res_n=res_n, model=model, **(SILU if eff else LIN))


def couts_with_ntw(H, W, k, s, ntw, lo=8, hi=520):
    """the output widths for which the launcher picks `ntw` column tiles per wave on this map (and the support check passes the
    projection's geometry)"""
    wi, _, _, _, mwp, _ = mb_geom(H, W)
    MTp = cdiv(conv_out(H, k, s) * conv_out(W, k, s), 16)
    out = []
    for cout in range(lo, hi, 8):
        NTp = cdiv(cout, 16)
        t = mb_pick_ntw(NTp, MTp, wi, mwp)
        nwn = cdiv(NTp, t)
        if t == ntw and nwn <= MB_WAVES and cdiv(MTp, min(MB_WAVES // nwn, MTp)) <= mwp:
            out.append(cout)
    return out


def _name(c: Case):
    kind = {(ACT_SILU, ACT_SILU, 0): "silu", (ACT_NONE, ACT_RELU, 1): "lin"}.get((c.act_d, c.se_act, c.a_relu6), f"d{c.act_d}se{c.se_act}r6{c.a_relu6}")
    return f"{c.H}x{c.W}_k{c.k}s{c.stride}_{kind}_c{c.Cin}_m{c.mid}_o{c.Cout}_rd{c.rd}_res{c.res_n}"


# edge cases: (map H, depthwise k, stride, expand k-steps, NTW, Cin = 32 kst - this, mid, rd, which of the widths that select NTW
# on this map (index, or "odd": the first with Cout % 16 == 8), residual "none" / "all" / "part", overrides).  W follows from the
# instance.  Each row exists for the SiLU family (efficientnet) and for the linear-depthwise family (rexnet) where the instance
# list has a counterpart; the coverage test lists what each edge needs.
_S14, _S14K5, _S14K5L, _S14S2 = (3, 1, 14, 3, 3), (5, 1, 14, 3, 3), (5, 1, 14, 5, 3), (5, 2, 14, 5, 2)
_S7W, _S7, _S7L = (5, 1, 7, 8, 2), (3, 1, 7, 8, 3), (3, 1, 7, 12, 3)
_L14N2, _L14, _L14K5, _L14K6, _L14N4 = (3, 1, 14, 4, 2), (3, 1, 14, 4, 3), (3, 1, 14, 5, 3), (3, 1, 14, 6, 3), (3, 1, 14, 6, 4)
_L7W7, _L7W, _L7, _L7K9, _L7K10, _L7K11 = (3, 1, 7, 7, 2), (3, 1, 7, 8, 2), (3, 1, 7, 8, 3), (3, 1, 7, 9, 3), (3, 1, 7, 10, 3), (3, 1, 7, 11, 3)
_EDGES_SILU = [
    # mid 8 / 120 / 128 / 136 (one slab: one wave, idle waves, none idle; a second slab with one active wave), rd 1 / 3 / 4 / 5 and
    # 16 JS / 16 JS + 1 (JS = 8), 173, 192
    (14, _S14, 0, 8, 1, 1, "none"), (14, _S14K5, 8, 120, 3, "odd", "part"), (14, _S14, 0, 128, 4, -1, "all"), (14, _S14K5L, 8, 136, 5, 0, "none"),
    (7, _S7W, 0, 8, 128, 1, "part"), (7, _S7, 24, 120, 129, "odd", "none"), (7, _S7L, 0, 128, 192, 1, "none"), (7, _S7W, 8, 136, 173, "odd", "all"),
    # JS = 2 (mid 1392 class) with rd 32 / 33, JS = 1 (mid >= 2056) with rd 16 / 17; the largest mid
    (7, _S7W, 24, 1400, 32, 0, "none"), (14, _S14, 0, 1392, 33, 0, "all"), (7, _S7L, 24, 2064, 16, -1, "part"), (14, _S14K5L, 8, 2056, 17, 0, "none"),
    (7, _S7, 24, 2560, 5, 0, "none"), (7, _S7W, 0, 2560, 4, "odd", "none"), (14, _S14K5, 24, 2560, 3, 1, "part"),
    # non-square maps: 5x7, 8x7 (the counted wait on a non-square map), 9x7; 10x14, 13x14; stride 2 from 10x14 and 13x14
    (5, _S7W, 0, 264, 18, 0, "all"), (9, _S7, 24, 264, 18, "odd", "none"), (5, _S7L, 8, 136, 18, 0, "none"), (8, _S7, 0, 392, 18, 2, "part"),
    (9, _S7W, 8, 2560, 18, -1, "none"), (9, _S7W, 0, 1400, 18, 0, "all"),
    (10, _S14, 8, 264, 18, "odd", "all"), (13, _S14K5, 0, 264, 18, -1, "none"), (10, _S14S2, 16, 264, 18, 0, "none"),
    (13, _S14S2, 24, 392, 18, "odd", "none"), (14, _S14S2, 24, 1392, 18, -1, "none"), (13, _S14K5L, 24, 1392, 18, 0, "part"),
    # the other SE activation and ReLU6 behind the gate on a SiLU-depthwise instance
    (14, _S14, 8, 264, 18, 0, "part", dict(se_act=ACT_RELU, a_relu6=1)), (7, _S7W, 8, 264, 18, 0, "none", dict(se_act=ACT_RELU, a_relu6=1)),
]
_EDGES_LIN = [
    (14, _L14, 0, 8, 1, 1, "none"), (14, _L14N2, 8, 120, 3, "odd", "part"), (14, _L14K5, 0, 128, 4, -1, "all"), (14, _L14K6, 8, 136, 5, 0, "none"),
    (7, _L7W, 0, 8, 128, 1, "part"), (7, _L7, 24, 120, 129, "odd", "none"), (7, _L7K11, 0, 128, 192, 1, "none"), (7, _L7W7, 8, 136, 173, "odd", "all"),
    (7, _L7W, 24, 1400, 32, 0, "none"), (14, _L14, 0, 1392, 33, 0, "all"), (7, _L7K10, 24, 2064, 16, -1, "part"), (14, _L14K6, 8, 2056, 17, 0, "none"),
    (7, _L7K9, 24, 2560, 5, 0, "none"), (7, _L7W7, 0, 2560, 4, "odd", "none"), (14, _L14N4, 24, 2560, 3, 1, "part"),
    (5, _L7W, 0, 264, 18, 0, "all"), (9, _L7, 24, 264, 18, "odd", "none"), (5, _L7K11, 8, 136, 18, 0, "none"), (8, _L7K9, 0, 392, 18, 2, "part"),
    (9, _L7W7, 8, 2560, 18, -1, "none"), (9, _L7W, 0, 1400, 18, 0, "all"),
    (10, _L14, 8, 264, 18, "odd", "all"), (13, _L14N2, 0, 264, 18, -1, "none"), (10, _L14N4, 16, 264, 18, 0, "none"),
    (13, _L14K5, 24, 392, 18, "odd", "none"), (13, _L14K6, 24, 1392, 18, 0, "part"),
    # the widths at which NTW flips on one instance family: 2 <-> 3 (Kp 128 at 14x14, Kp 256 at 7x7) and 3 <-> 4 (Kp 192 at 14x14)
    (14, _L14, 0, 264, 18, 96, "none"), (14, _L14N2, 0, 264, 18, 104, "none"), (14, _L14N2, 0, 264, 18, 128, "none"), (14, _L14, 0, 264, 18, 136, "none"),
    (14, _L14K6, 0, 264, 18, 192, "none"), (14, _L14N4, 0, 264, 18, 200, "none"),
    (7, _L7W, 0, 264, 18, 48, "none"), (7, _L7, 0, 264, 18, 56, "none"), (7, _L7, 0, 264, 18, 192, "none"), (7, _L7W, 0, 264, 18, 200, "none"),
    (7, _L7W, 0, 264, 18, 256, "none"), (7, _L7, 0, 264, 18, 264, "none"),
    # the other SE activation and no ReLU6 on a linear-depthwise instance
    (14, _L14, 8, 264, 18, 0, "part", dict(se_act=ACT_SILU, a_relu6=0)), (7, _L7W, 8, 264, 18, 0, "none", dict(se_act=ACT_SILU, a_relu6=0)),
]


def _edge(row, ad):
    H, (k, s, wi, kst, ntw), cmod, mid, rd, pick, res = row[:7]
    over = row[7] if len(row) > 7 else {}
    cin = 32 * kst - cmod
    couts = couts_with_ntw(H, wi, k, s, ntw)
    cout = pick if isinstance(pick, int) and pick >= 8 else (next(c for c in couts if c % 16 == 8) if pick == "odd" else couts[pick])
    assert cout in couts, (row, couts)
    m = min(cin, cout)
    res_n = 0 if res == "none" or s == 2 else (m if res == "all" or m == 8 else (m // 2) & ~7)
    kind = dict(SILU if ad == ACT_SILU else LIN)
    kind.update(over)
    return Case(H, wi, cin, mid, cout, k, s, rd, res_n=res_n, **kind)


def _cases():
    C = {}
    for L in MODEL_LAYERS:
        model, m, cin, mid, cout, k, s, rd, _ = L
        C[f"model_{model}_{cin}_{mid}_{cout}_k{k}s{s}_at{m}"] = model_case(*L)

    # ---- every instance on its class's square map, small: mid 264 = three slabs (the last holds one active wave with half a
    # tile), rd 18 = five FC1 groups with a tail of two, Cin % 32 dealt round {0, 8, 24}, Cout the smallest and the largest
    # width that selects the instance's NTW, a residual over all / a part / none of the columns.  The batch-position test repeats
    # the second of each pair (several column groups in the projection) with ROT_B copies of one image.
    for i, (k, s, wi, kst, ntw, ad) in enumerate(INSTANCES):
        kind = SILU if ad == ACT_SILU else LIN
        couts = couts_with_ntw(wi, wi, k, s, ntw)
        for j, cout in enumerate((couts[0], couts[-1])):
            cin = next(ci for ci in (32 * kst - (0, 8, 24, 16)[(i + j + t) % 4] for t in range(4))
                       if mbconv_block_supported(wi, wi, ci, 264, cout, k, s, 18, ACT_SILU, ad))
            m = min(cin, cout)
            res_n = 0 if s == 2 else (0, m, (m // 2) & ~7)[(i + j) % 3]
            c = Case(wi, wi, cin, 264, cout, k, s, 18, res_n=res_n, **kind)
            C[f"inst{i:02d}{'ab'[j]}_" + _name(c)] = c
    for ad, rows in ((ACT_SILU, _EDGES_SILU), (ACT_NONE, _EDGES_LIN)):
        for row in rows:
            c = _edge(row, ad)
            C["edge_" + _name(c)] = c
    return C


def rotation_cases():
    """one case per instance for the batch-position test: ROT_B copies of one image"""
    return {n: replace(c, B=ROT_B, same=True) for n, c in CASES.items() if n.startswith("inst") and n[6] == "b"}


CASES = _cases()


# ------------------------------------------------------------------------------------------------------ data (CPU, seeded)
def _bf(t):
    return t.to(torch.bfloat16).float()


class Data:
    """Seeded operands of one case (imageretrievalresearch_amd.synth streams); bf16 values held in fp32.  x, we, be, wd, bd are
    what mbconv_front_ref.reference reads.

    Every sum in front of the gate is COHERENT: the terms of one sum share their sign (a sign per expanded channel for the expand
    weights, the depthwise taps and the SE reduce weights, a sign per hidden unit, a sign per gate channel), with 50 % noise on
    every factor.  The worst-case magnitudes behind dg (sum |x| |w| and on through both FCs) then stay within a small factor of the
    values themselves, dg / g stays near 2^-17, and about 1 % of the A' elements are flippable; with random signs the magnitudes
    are sqrt(Cin), sqrt(mid) and sqrt(rd) times the values and nearly every A' element would be.  What tells pixels, channels,
    hidden units and images apart is a factor of their own on each: a scale per image (0.6 .. 1.1) and per pixel (0.4 .. 1.6), per
    expanded channel (0.6 .. 1.8, negative for a quarter), per tap, and per gate channel (pre-sigmoid spread about +-2, and the
    gates of two images differ by several per cent).  The first and last 8 expanded channels and the first and last hidden unit
    carry about a tenth of their FC's sum each (harmonic profiles), so that losing one of them is visible.  With ReLU6 behind the
    gate the depthwise side is scaled by 3: D reaches past 6."""

    def __init__(self, c: Case):
        seed = 90000 + 64 * (c.H * 131 + c.W * 17 + c.Cin * 3 + c.mid * 11 + c.Cout * 7 + c.k + 5 * c.stride + c.rd * 13 + c.seed * 977)
        n = lambda i, *shape: torch.from_numpy(synth.normal(seed + i, shape).astype(np.float32))       # noqa: E731
        u = lambda i, *shape: torch.from_numpy(synth.uniform(seed + i, shape).astype(np.float32))      # noqa: E731
        sign = lambda i, p, *shape: torch.where(u(i, *shape) < p, 1.0, -1.0)                           # noqa: E731
        b = torch.arange(c.B)
        scale = 0.6 + 0.5 * ((b * 7) % 13).float() / 13 + 0.002 * b.float()
        alpha = scale[:, None, None] * (0.4 + 1.2 * u(20, c.B, c.H, c.W))
        x = alpha[..., None] * (1.0 + 0.5 * n(0, c.B, c.H, c.W, c.Cin))
        if c.same:
            x[:] = x[0].clone()
        self.x = _bf(x)
        sb = sign(21, 0.75, c.mid)                                       # sign of an expanded channel's E
        beta = sb * (0.6 + 1.2 * u(22, c.mid))
        self.we = _bf(beta[:, None] * (1.0 + 0.5 * n(1, c.mid, c.Cin)) * (1.5 / c.Cin))
        self.be = sb * n(2, c.mid).abs() * 0.3
        ds = 3.0 if c.a_relu6 else 1.0
        sd = sign(23, 0.7, c.mid)                                        # sign of a channel's taps
        self.wd = _bf(sd * (1.0 + 0.5 * n(3, c.k * c.k, c.mid)) * (1.2 * ds / (c.k * c.k)))        # [k*k][mid], tap ky * k + kx
        self.bd = sd * sb * n(4, c.mid).abs() * 0.3 * ds
        # SE: hidden units about +-1, the active ones (three quarters) near 1 behind SiLU / ReLU; pre-sigmoid within about +-2.5
        prof = lambda m, g: 1.0 / (1.0 + torch.minimum(torch.arange(m), m - 1 - torch.arange(m)) // g)  # noqa: E731
        pn = prof(c.mid, 8)
        sj = sign(24, 0.75, c.rd)
        sj[0] = sj[-1] = 1.0
        s_nom = ds * (0.8 if c.act_d == ACT_SILU else 1.25)              # |squeeze|, roughly
        self.w1 = _bf(sj[:, None] * (sd * sb * pn)[None, :] * (0.5 + u(5, c.rd, c.mid)) * (1.1 / s_nom / pn.sum()))
        self.b1 = sj * n(6, c.rd).abs() * 0.2
        qj = prof(c.rd, 1)
        cn = (2.0 * u(7, c.mid) - 1.0) * 1.8                             # pre-sigmoid value of a gate channel, roughly
        self.w2 = _bf(cn[None, :] * qj[:, None] * (0.5 + u(8, c.rd, c.mid)) / qj.sum())
        self.b2 = n(9, c.mid) * 0.3
        self.wp = _bf(n(10, c.Cout, c.mid) * (2.0 / ds / math.sqrt(c.mid)))
        self.bp = n(11, c.Cout) * 0.3

    def we_packed(self, c: Case):
        """[ceil16(mid)][ceil32(Cin)] zero padded (GEMM packing), and the bias [ceil16(mid)]"""
        return _packed(self.we, self.be)

    def wp_packed(self, c: Case):
        """[ceil16(Cout)][ceil32(mid)] zero padded, and the bias [ceil16(Cout)]"""
        return _packed(self.wp, self.bp)


def _packed(w, b):
    wp = torch.zeros((w.shape[0] + 15) // 16 * 16, kpad32(w.shape[1]))
    wp[:w.shape[0], :w.shape[1]] = w
    bp = torch.zeros(wp.shape[0])
    bp[:b.shape[0]] = b
    return wp, bp


# ------------------------------------------------------------------------------------------------------------ reference
@dataclass
class Front:
    """the float64 front half of one case: computed once, shared, never changed"""
    d64: torch.Tensor           # [B][Ho][Wo][mid] un-rounded act_d values
    tolD: torch.Tensor
    s64: torch.Tensor           # [B][mid] squeeze (mean over the map)
    ds: torch.Tensor            # its bound
    share_e: float              # flippable share of the E elements


def front(c: Case, d: Data):
    res, share = front_reference(c.front, d)
    return Front(res["D"][0], res["D"][1], res["pool"][0], res["pool"][1], share)


def _relu6(a, on):
    return a.clamp(0.0, 6.0) if on else a


def _residual(c: Case, d: Data, n):
    """[B][Pout][Cout] float64: X on the first n output columns (stride 1: the output pixel is the input pixel)"""
    r = torch.zeros(c.B, c.Pout, c.Cout, dtype=torch.float64)
    if n:
        idx = torch.arange(n) % c.Cin            # (a column past Cin exists only in a mutant)
        r[..., :n] = d.x.double().view(c.B, c.H * c.W, c.Cin)[..., idx]
    return r


def gate(c: Case, d: Data, s):
    """float64 gate [B][mid] of the squeeze s, and the hidden vector"""
    r = _act(s @ d.w1.double().t() + d.b1.double(), c.se_act)
    return torch.sigmoid(r @ d.w2.double() + d.b2.double()), r


def tail(c: Case, d: Data, fr: Front, Dk):
    """Y's reference and tolerance from the kernel's own depthwise output Dk [B][Ho][Wo][mid] (exact bf16 values, float64).
    -> dict(y [B][Ho][Wo][Cout], tol, terms = the tolerance's three parts, share_a, g, dg)"""
    w1, b1, w2, b2 = d.w1.double(), d.b1.double(), d.w2.double(), d.b2.double()
    g, _ = gate(c, d, fr.s64)
    mag_s = fr.ds / TOL_SE
    mag_r = DERIV[c.se_act] * (mag_s @ w1.abs().t() + b1.abs())
    mag_g = 0.25 * (mag_r @ w2.abs() + b2.abs())
    dg = TOL_SE * (mag_g + g.abs())
    Dk = Dk.reshape(c.B, c.Pout, c.mid)
    a64 = _relu6(Dk * g[:, None, :], c.a_relu6)
    a_r = round_bf16(a64)
    flip = midpoint_distance(a64) <= Dk.abs() * dg[:, None, :] + TOL_MUL * a64.abs()
    slack = torch.where(flip, ulp_bf16(a64), torch.zeros_like(a64))
    wp, bp = d.wp.double(), d.bp.double()
    res = _residual(c, d, c.res_n)
    y = a_r @ wp.t() + bp + res
    magY = a_r.abs() @ wp.abs().t() + bp.abs() + res.abs()
    terms = torch.stack([TOL_REL * y.abs(), TOL_ACC * magY, slack @ wp.abs().t()])
    sh = (c.B, c.Ho, c.Wo, c.Cout)
    return dict(y=y.view(sh), tol=terms.sum(0).view(sh), terms=terms.view(3, *sh), share_a=flip.double().mean().item(), g=g, dg=dg)


TERMS = ("2^-8 |y64| (the bf16 rounding of Y)", "2^-20 magY (fp32 accumulation)", "slack of the flippable A' elements")


# -------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = {
    "squeeze_divided_by_input_hw": lambda c: c.stride == 2,
    "gate_from_neighbour_image": lambda c: c.B > 1 and not c.same,
    "gate_chunk_from_neighbour_image": lambda c: c.B > 1 and not c.same,
    "hidden_unit_last_dropped": lambda c: True,
    "squeeze_misses_last_8_channels": lambda c: True,
    "projection_k_misses_last_8_channels": lambda c: True,
    "b2_omitted": lambda c: True,
    "w2_read_untransposed": lambda c: c.rd > 1,
    "relu6_omitted": lambda c: c.a_relu6 == 1,
    "relu6_before_the_gate": lambda c: c.a_relu6 == 1,
    "residual_omitted": lambda c: c.res_n > 0,
    "residual_on_every_column": lambda c: 0 < c.res_n < c.Cout,
    "last_pixel_row_from_the_row_above": lambda c: c.Ho > 1,
    "taps_transposed": lambda c: True,
    "last_8_output_channels_zero": lambda c: True,
}


def mutant_outputs(c: Case, d: Data, fr: Front, mut):
    """(D, Y) float64 holding bf16 values: what a kernel with the named bug, otherwise exact, would write."""
    v = fr.d64
    if mut == "taps_transposed":
        v = front_reference(c.front, d, "taps_transposed")[0]["D"][0]
    if mut == "last_pixel_row_from_the_row_above":
        v = v.clone()
        v[:, -1] = v[:, -2]
    D = round_bf16(v)
    s = v.mean((1, 2))
    if mut == "squeeze_divided_by_input_hw":
        s = s * (c.Pout / (c.H * c.W))
    if mut == "squeeze_misses_last_8_channels":
        s = s.clone()
        s[:, -8:] = 0.0
    w1, b1, w2, b2 = d.w1.double(), d.b1.double(), d.w2.double(), d.b2.double()
    if mut == "hidden_unit_last_dropped":
        w2 = w2.clone()
        w2[-1] = 0.0
    if mut == "b2_omitted":
        b2 = torch.zeros_like(b2)
    if mut == "w2_read_untransposed":
        w2 = w2.reshape(c.mid, c.rd).t()
    r = _act(s @ w1.t() + b1, c.se_act)
    g = torch.sigmoid(r @ w2 + b2)
    nb = torch.tensor([i + 1 if i + 1 < c.B else i - 1 for i in range(c.B)])
    if mut == "gate_from_neighbour_image":
        g = g[nb]
    if mut == "gate_chunk_from_neighbour_image":
        g = g.clone()
        # the first chunk from the middle on that ReLU6 does not wipe out (linear depthwise: half the channels are negative)
        live = ((v[0].reshape(-1, c.mid // 8, 8) > 0).any(0).sum(1) >= 4).roll(-(c.mid // 16), 0)
        lo = (int(live.int().argmax()) + c.mid // 16) % (c.mid // 8) * 8
        g[:, lo:lo + 8] = g[nb, lo:lo + 8]
    Dp = D.reshape(c.B, c.Pout, c.mid)
    if mut == "relu6_omitted":
        a = Dp * g[:, None, :]
    elif mut == "relu6_before_the_gate":
        a = _relu6(Dp, True) * g[:, None, :]
    else:
        a = _relu6(Dp * g[:, None, :], c.a_relu6)
    a = round_bf16(a)
    if mut == "projection_k_misses_last_8_channels":
        a[..., -8:] = 0.0
    n = {"residual_omitted": 0, "residual_on_every_column": c.Cout}.get(mut, c.res_n)
    y = a @ d.wp.double().t() + d.bp.double() + _residual(c, d, n)
    if mut == "last_8_output_channels_zero":
        y[..., -8:] = 0.0
    return D, round_bf16(y).view(c.B, c.Ho, c.Wo, c.Cout)
