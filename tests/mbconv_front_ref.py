"""Float64 reference, tolerances, dispatch rules and cases for the fused expand + depthwise kernels (k_fused_late and k_fused_band,
csrc/fused_mbconv.hip; k_sweep_mbconv, csrc/sweep_mbconv.hip), reached through the developer entry mi355_mbconv_front_ex.
Plain torch / numpy on the CPU; tests/test_mbconv_front_gpu.py holds the tests.

Rounding points of the three kernels (they agree):
    E = bf16(act_e(fp32 MFMA sum + be))      lives only in the LDS
    D = bf16(act_d(fp32 tap sum + bd))
    squeeze = sum of the un-rounded fp32 act_d values

E cannot be read back, and the kernel's fp32 sum can land on the other side of a bf16 rounding boundary from the float64 value.
The reference therefore rounds the float64 E itself (e_r: round to nearest even on the float64 value, never via float32), and
gives every E element that lies within dE = 2^-20 magE of a midpoint between two bf16 neighbours ("flippable") one bf16 ulp of
slack, which is carried through the depthwise taps:
    magE = deriv_e (sum |x| |w| + |be|)                      2^-20: the fp32-accumulation coefficient of test_gemm_paths_gpu.py
    d64  = act_d(sum_taps e_r wd + bd), zero padding         magD = sum |e_r| |wd| + |bd|
    |D - d64|                  <= 2^-8 |d64| + deriv_d (2^-18 magD + sum_taps |wd| slack)
    |pool / (Ho Wo) - mean d64| <= 2^-18 mean(deriv_d magD) + mean(deriv_d sum_taps |wd| slack)
2^-8 is the one bf16 rounding of D, 2^-18 the fp32 sum of at most 26 terms plus the activation (test_conv_paths_gpu.py); the squeeze
term is the same STATISTICAL fp32 bound as there (a correct kernel that exceeded it would call for the worst-case n 2^-24 term,
not a looser coefficient).  The flippable share of a case's E elements must stay at or below FLIP_CAP."""
import math
from dataclasses import dataclass

import numpy as np
import torch

TOL_REL = 2.0 ** -8
TOL_DW = 2.0 ** -18
TOL_E = 2.0 ** -20
FLIP_CAP = 0.05
MARGIN = 10.0
GUARD = 256                 # NaN elements behind D and pool: an overrun lands there
ACT_NONE, ACT_SILU, ACT_RELU, ACT_RELU6, ACT_GELU, ACT_SIGMOID = range(6)
DERIV = {ACT_NONE: 1.0, ACT_SILU: 1.1, ACT_RELU: 1.0, ACT_RELU6: 1.0, ACT_GELU: 1.13, ACT_SIGMOID: 0.25}

# include/mi355_retrieval.h (test_path_enum_matches_the_header keeps the two in step)
KERNELS = {"auto": 0, "late": 1, "sweep": 2, "band": 3}
ACT_INST = {"SILU_SILU": 1, "SILU_NONE": 2, "RUNTIME": 3}
SWEEP_CLASS = {"3_2_112": 1, "3_1_56": 2, "5_2_56": 3, "5_1_28": 4, "3_2_28": 5, "3_2_56": 6, "3_1_28": 7}
FL_THREADS = 512


def cdiv(a, b):
    return -(-a // b)


def kpad32(k):
    return (k + 31) & ~31


def path_base(family, k, s):
    return KERNELS[family] | (k == 5) << 2 | (s == 2) << 3


def path_late(k, s, niw, px):
    return path_base("late", k, s) | niw << 4 | px << 8


def path_band(k, s, kst, px, mc, th):
    return path_base("band", k, s) | kst << 4 | px << 8 | mc << 12 | th << 20


def path_sweep(k, s, cls, kst, ns, variant, act, csplit):
    return path_base("sweep", k, s) | cls << 4 | kst << 8 | ns << 12 | variant << 14 | act << 17 | csplit << 19


# ------------------------------------------------------------------------------------- the launchers' rules, written out
def conv_out(h, k, s):
    return (h + 2 * (k // 2) - k) // s + 1


def _px(W, k, s):
    return 7 if conv_out(W, k, s) % 7 == 0 else 4


def late_niw(H, W):
    return 4 if H * W <= 64 else (2 if H * W <= 112 else 1)


def late_lds_bytes(H, W, Kp, MC, k, s):
    P, pad = H * W, k // 2
    MT = cdiv(P, 16)
    iw = (_px(W, k, s) - 1) * s + k
    EP = H * (W + 2 * pad) + iw
    return MT * 16 * (Kp + 8) * 2 + ((EP + 7) & ~7) * (MC + 8) * 2 + FL_THREADS * 8 * 4


def late_supported(H, W, Cin, mid, k, s):
    if H * W > 208 or Cin % 8 or mid % 8 or k not in (3, 5) or s not in (1, 2):
        return False
    return late_lds_bytes(H, W, kpad32(Cin), 128 * late_niw(H, W), k, s) <= 160 * 1024


def band_slab(mid):
    return 64 if mid % 64 == 0 else (48 if mid % 48 == 0 else 64)


def band_lds_bytes(W, Kp, k, s, TH, px, mc):
    pad, IH = k // 2, (TH - 1) * s + k
    MT = cdiv(IH * W, 16)
    EP = IH * (W + 2 * pad) + (px - 1) * s + k
    return MT * 16 * (Kp + 8) * 2 + ((EP + 7) & ~7) * (mc + 8) * 2 + FL_THREADS * 8 * 4


def band_rows_max(H, W, Cin, mid, k, s):
    """fused_band_rows: the largest band height whose LDS image fits, 0 = unsupported."""
    if Cin % 8 or mid % 8 or Cin > 64 or W > 128 or k not in (3, 5) or s not in (1, 2):
        return 0
    Ho, best = conv_out(H, k, s), 0
    for th in range(1, min(Ho, 16) + 1):
        if band_lds_bytes(W, kpad32(Cin), k, s, th, _px(W, k, s), band_slab(mid)) <= 158 * 1024:
            best = th
    return best


SW_GEOM = {1: (3, 2, 112), 2: (3, 1, 56), 3: (5, 2, 56), 4: (5, 1, 28), 5: (3, 2, 28), 6: (3, 2, 56), 7: (3, 1, 28)}   # k, s, map
# (TH, NW, OCC) of variant 0 and of the tuning variants 1..4 of the generic classes (SW_V0 / SW_VT of launch_sweep_mbconv)
SW_V0 = {1: (2, 8, 2), 2: (8, 8, 2), 3: (2, 7, 2), 4: (4, 7, 2), 5: (4, 7, 2)}
SW_VT = {1: {1: (2, 7, 2), 2: (2, 8, 3), 3: (1, 7, 2), 4: (1, 4, 4)},
         2: {1: (8, 7, 2), 2: (4, 8, 2), 3: (2, 7, 2), 4: (2, 7, 3)},
         3: {1: (4, 7, 2), 2: (2, 8, 2), 3: (2, 7, 2), 4: (1, 7, 2)},
         4: {1: (4, 7, 2), 2: (4, 8, 2), 3: (2, 7, 2), 4: (4, 4, 4)},
         5: {1: (7, 7, 2), 2: (4, 8, 2), 3: (2, 7, 2), 4: (4, 7, 2)}}
SW_VT_KST = {1: 1, 2: 1, 3: 1, 4: 2, 5: 2}            # the k-steps the tuning variants exist for
# RexNet instances (SiLU / none): (class, k-steps) -> (TH, NW, OCC, NS); and their variant-3 one-tile forms
SW_REX = {(2, 2): (8, 8, 1, 2), (6, 2): (2, 7, 1, 2), (6, 3): (2, 7, 1, 2), (7, 3): (4, 7, 2, 1), (7, 4): (4, 7, 2, 1),
          (5, 3): (4, 7, 2, 1)}
SW_REX_V3 = {(2, 2): (8, 8, 1, 1), (6, 2): (2, 7, 1, 1), (6, 3): (2, 7, 2, 1)}


def sweep_class(H, W, k, s):
    for cls, (kk, ss, m) in SW_GEOM.items():
        if (k, s, H, W) == (kk, ss, m, m):
            return cls
    return 0


def sweep_rex_instance(cls, kst):
    return (cls, kst) in SW_REX and (cls, kst) != (2, 2)


def sweep_supported(H, W, Cin, mid, k, s, act_e, act_d):
    if Cin % 8 or mid % 8 or Cin < 8:
        return False
    cls, kst = sweep_class(H, W, k, s), cdiv(Cin, 32)
    if cls == 0:
        return False
    if act_e == ACT_SILU and act_d == ACT_NONE and sweep_rex_instance(cls, kst):
        return True
    return Cin <= 64 and cls <= 5


def sweep_instance(H, W, Cin, k, s, act_e, act_d, variant):
    """launch_sweep_mbconv's choice: dict(cls, kst, ns, variant (the one that ran), act, TH, NW, OCC)."""
    cls, kst = sweep_class(H, W, k, s), kpad32(Cin) // 32
    if act_e == ACT_SILU and act_d == ACT_NONE and (cls, kst) in SW_REX:
        v = 3 if variant == 3 and (cls, kst) in SW_REX_V3 else 0
        TH, NW, OCC, NS = (SW_REX_V3 if v else SW_REX)[(cls, kst)]
        return dict(cls=cls, kst=kst, ns=NS, variant=v, act=ACT_INST["SILU_NONE"], TH=TH, NW=NW, OCC=OCC)
    assert kst <= 2 and cls <= 5
    silu = act_e == ACT_SILU and act_d == ACT_SILU
    v = variant if silu and kst == SW_VT_KST[cls] and 1 <= variant <= 4 else 0
    TH, NW, OCC = SW_VT[cls][v] if v else SW_V0[cls]
    act = "SILU_SILU" if silu else ("SILU_NONE" if (act_e, act_d) == (ACT_SILU, ACT_NONE) else "RUNTIME")
    return dict(cls=cls, kst=kst, ns=1, variant=v, act=ACT_INST[act], TH=TH, NW=NW, OCC=OCC)


def sweep_csplit(W, mid, B, ns, occ, override):
    """launch_sw_act: workgroups per image."""
    nslab = cdiv(cdiv(mid, 16), ns)
    if override > 0:
        return min(override, nslab)
    c = (3 if W == 112 else 4) if W >= 56 else 2
    while c < nslab and (nslab % c != 0 or B * c < 256 * occ):
        c += 1
    return min(c, nslab)


def auto_family(H, W, Cin, mid, k, s, act_e, act_d):
    """fused_pair_shape_how under the model's default options (fuse_sweep 1, fuse_band 2): "late" / "sweep" / "band" / None."""
    if late_supported(H, W, Cin, mid, k, s):
        return "late"
    if sweep_supported(H, W, Cin, mid, k, s, act_e, act_d):
        return "sweep"
    rows = band_rows_max(H, W, Cin, mid, k, s)
    if rows > 0 and k == 3 and ((s == 1 and rows >= 7) or (s == 2 and W >= 112 and mid >= 192)):
        return "band"
    return None


def reachable_instances():
    """Every template instance the three launchers can select: ("late", k, s, NIW, PX), ("band", k, s, KST, PX, MC),
    ("sweep", class, KST, NS, variant, activation instance)."""
    ks = [(k, s) for k in (3, 5) for s in (1, 2)]
    out = {("late", k, s, niw, px) for k, s in ks for niw in (4, 2, 1) for px in (7, 4)}
    out |= {("band", k, s, kst, px, mc) for k, s in ks for kst in (1, 2) for px in (7, 4) for mc in (48, 64)}
    for cls in SW_V0:
        for kst in (1, 2):
            for act in ACT_INST.values():
                if (cls, kst) in SW_REX and act == ACT_INST["SILU_NONE"]:
                    continue                                       # 3_1_56 with two k-steps: the RexNet instance takes it
                out.add(("sweep", cls, kst, 1, 0, act))
        out |= {("sweep", cls, SW_VT_KST[cls], 1, v, ACT_INST["SILU_SILU"]) for v in (1, 2, 3, 4)}
    out |= {("sweep", cls, kst, t[3], 0, ACT_INST["SILU_NONE"]) for (cls, kst), t in SW_REX.items()}
    out |= {("sweep", cls, kst, t[3], 3, ACT_INST["SILU_NONE"]) for (cls, kst), t in SW_REX_V3.items()}
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    kernel: str                 # the `kernel` argument: "late" / "sweep" / "band" (forced) or "auto"
    B: int
    H: int
    W: int
    Cin: int
    mid: int
    k: int
    stride: int
    act_e: int = ACT_SILU
    act_d: int = ACT_SILU
    band_rows: int = 0
    variant: int = 0
    csplit: int = 0
    pool: bool = True
    dup: tuple = ()             # (i, j): image j repeats image i and must come out with identical bits
    seed: int = 0

    @property
    def Ho(self):
        return (self.H - 1) // self.stride + 1

    @property
    def Wo(self):
        return (self.W - 1) // self.stride + 1

    @property
    def family(self):
        if self.kernel != "auto":
            return self.kernel
        return auto_family(self.H, self.W, self.Cin, self.mid, self.k, self.stride, self.act_e, self.act_d)

    @property
    def supported(self):
        a = (self.H, self.W, self.Cin, self.mid, self.k, self.stride)
        if self.family == "late":
            return late_supported(*a)
        if self.family == "sweep":
            return sweep_supported(*a, self.act_e, self.act_d)
        return self.family == "band" and 0 <= self.band_rows <= band_rows_max(*a)

    @property
    def sweep(self):
        return sweep_instance(self.H, self.W, self.Cin, self.k, self.stride, self.act_e, self.act_d, self.variant)

    @property
    def TH(self):
        """output rows per band (band and sweep kernels); the whole image for the late kernel"""
        if self.family == "band":
            return self.band_rows or band_rows_max(self.H, self.W, self.Cin, self.mid, self.k, self.stride)
        return self.sweep["TH"] if self.family == "sweep" else self.Ho

    @property
    def slab(self):
        """channels per slab"""
        if self.family == "late":
            return 128 * late_niw(self.H, self.W)
        return band_slab(self.mid) if self.family == "band" else 16 * self.sweep["ns"]

    @property
    def nblk(self):
        return cdiv(self.Ho, self.TH) if self.family == "band" else 1

    @property
    def used_csplit(self):
        i = self.sweep
        return sweep_csplit(self.W, self.mid, self.B, i["ns"], i["OCC"], self.csplit)

    @property
    def instance(self):
        k, s = self.k, self.stride
        if self.family == "late":
            return ("late", k, s, late_niw(self.H, self.W), _px(self.W, k, s))
        if self.family == "band":
            return ("band", k, s, kpad32(self.Cin) // 32, _px(self.W, k, s), band_slab(self.mid))
        i = self.sweep
        return ("sweep", i["cls"], i["kst"], i["ns"], i["variant"], i["act"])

    @property
    def code(self):
        """the `path` the entry must report"""
        t = self.instance
        if t[0] == "late":
            return path_late(*t[1:])
        if t[0] == "band":
            return path_band(*t[1:], self.TH)
        return path_sweep(self.k, self.stride, *t[1:], self.used_csplit)


def _widest_band_w(H, Cin, mid, k, s):
    """the widest map the band kernel's LDS check admits for this layer"""
    return max(w for w in range(8, 129) if band_rows_max(H, w, Cin, mid, k, s) > 0)


def _cases():
    C = {}
    KS = [(3, 1), (5, 1), (3, 2), (5, 2)]
    # ---- k_fused_late<KS, S, NIW, PX>: 24 instances.  Wo % 7 == 0 selects PX 7, otherwise PX 4 (a partial last strip but for 13x15 s2).
    # Cin 8 and Cin % 32 != 0 (Kp padding), mid % 16 == 8, mid = 128 NIW + 8 (the second slab holds one channel group)
    cins, i = [8, 24, 40, 72, 104, 16], 0
    for k, s in KS:
        for niw, (h7, w7), (h4, w4) in ((4, (4, 14) if s == 2 else (7, 7), (5, 9)), (2, (8, 14), (9, 11)), (1, (14, 14), (13, 15))):
            for px, (H, W) in ((7, (h7, w7)), (4, (h4, w4))):
                mid = (128 * niw + 8, 72, 136, 128 * niw)[i % 4]
                C[f"late_k{k}s{s}_niw{niw}_px{px}_{H}x{W}_c{cins[i % 6]}_m{mid}"] = Case("late", 3, H, W, cins[i % 6], mid, k, s,
                                                                                       act_d=ACT_NONE if i % 5 == 4 else ACT_SILU)
                i += 1
    # one slab per workgroup (B = 3, above); G = 2 with 2 + 1 slabs per workgroup, start rotated by image (B = 100); G = 1 with three
    # slabs and every rotation (B = 130, more images than slabs)
    C["late_b100_14x14_c16_m264"] = Case("late", 100, 14, 14, 16, 264, 3, 1, dup=(5, 78))
    C["late_b130_5x5_c24_m1032"] = Case("late", 130, 5, 5, 24, 1032, 5, 1, dup=(1, 129))
    # the models' own layers
    for name, (H, cin, mid, k, s, ad) in {
            "eff_96_576_k3": (14, 96, 576, 3, 1, ACT_SILU), "eff_96_576_k5": (14, 96, 576, 5, 1, ACT_SILU),
            "eff_136_816_k5s1": (14, 136, 816, 5, 1, ACT_SILU), "eff_136_816_k5s2": (14, 136, 816, 5, 2, ACT_SILU),
            "eff_232_1392_k5": (7, 232, 1392, 5, 1, ACT_SILU), "eff_232_1392_k3": (7, 232, 1392, 3, 1, ACT_SILU),
            "eff_384_2304_k3": (7, 384, 2304, 3, 1, ACT_SILU), "rex_108_648": (14, 112, 648, 3, 1, ACT_NONE),
            "rex_352_2088": (7, 352, 2088, 3, 1, ACT_NONE)}.items():
        C[f"late_{name}_at{H}"] = Case("late", 3, H, H, cin, mid, k, s, act_d=ad)

    # ---- k_fused_band<KS, S, KST, PX, MC>: 32 instances on 10x14 (PX 7) and 9x13 / 9x12 (PX 4, partial last strip) maps; mid 144 ->
    # MC 48 (NACT = 510: two threads idle in the reduction), 192 -> MC 64; band_rows 1, the default (one band: its halo lies outside
    # the image above and below), 3 and 4 (Ho % TH != 0)
    i = 0
    for k, s in KS:
        for kst, cin in ((1, 24), (2, 40)):
            for px, (H, W) in ((7, (10, 14)), (4, (9, 12) if s == 2 else (9, 13))):
                for mc, mid in ((48, 144), (64, 192)):
                    rows = (1, 0, 3, 4)[i % 4]
                    rows = min(rows, conv_out(H, k, s))
                    C[f"band_k{k}s{s}_kst{kst}_px{px}_mc{mc}_{H}x{W}_th{rows}"] = Case(
                        "band", 2, H, W, cin, mid, k, s, band_rows=rows, act_e=(ACT_SILU, ACT_RELU6)[i % 7 == 3],
                        act_d=(ACT_SILU, ACT_NONE, ACT_RELU6)[i % 3])
                    i += 1
    C["band_m200_partial_slab_11x14"] = Case("band", 2, 11, 14, 24, 200, 3, 1, band_rows=4)
    C["band_m200_partial_slab_k5s2_9x12"] = Case("band", 2, 9, 12, 40, 200, 5, 2, band_rows=2)
    C["band_w128_k3s1"] = Case("band", 2, 5, 128, 24, 144, 3, 1)
    w = _widest_band_w(6, 40, 192, 5, 2)
    C[f"band_widest_k5s2_6x{w}"] = Case("band", 2, 6, w, 40, 192, 5, 2)
    C["band_model_32_192_k3s1_at56"] = Case("band", 2, 56, 56, 32, 192, 3, 1)
    C["band_model_32_192_k3s2_at112"] = Case("band", 2, 112, 112, 32, 192, 3, 2, act_d=ACT_NONE)

    # ---- k_sweep_mbconv: the generic classes x Kp {32, 64} x {SiLU/SiLU, SiLU/none, ReLU6/ReLU6}; (3_1_56, Kp 64, SiLU/none) is the
    # RexNet instance.  Edges are dealt round the cases: B 1 / 2 / 3 / 9 (a grid padded to 16 images), mid % 16 == 8, pool null,
    # csplit forced to the B = 256 value (3 at 112, 4 at 56, 2 at 28: a workgroup walks several slabs from its image-dependent
    # start) and to a value that does not divide the slab count.
    b256 = {112: 3, 56: 4, 28: 2}
    i = 0
    for cls in range(1, 6):
        k, s, m = SW_GEOM[cls]
        for cin in (24, 40):
            for ae, ad, an in ((ACT_SILU, ACT_SILU, "ss"), (ACT_SILU, ACT_NONE, "sn"), (ACT_RELU6, ACT_RELU6, "rt")):
                B = (2, 1, 3, 9, 2, 2)[i % 6] if m > 28 else (3, 1, 2, 9, 4, 2)[i % 6]
                mid, cs = [(48, 0), (40, 0), (16 * 3 * b256[m], b256[m]), (24, 0), (112, b256[m] + 1 if m == 56 else b256[m]), (32, 0)][i % 6]
                C[f"sweep_{k}_{s}_{m}_c{cin}_{an}_b{B}_m{mid}_cs{cs}"] = Case("sweep", B, m, m, cin, mid, k, s, act_e=ae, act_d=ad, csplit=cs,
                                                                          pool=i % 6 != 5, dup=(0, B - 1) if cs and B > 1 else ())
                i += 1
    # tuning variants 1..4 of each generic class (set_option("sweep_variant"))
    for cls in range(1, 6):
        k, s, m = SW_GEOM[cls]
        for v in (1, 2, 3, 4):
            C[f"sweep_{k}_{s}_{m}_variant{v}"] = Case("sweep", 2, m, m, 32 * SW_VT_KST[cls] - 8, (40, 48, 24, 64)[v - 1], k, s, variant=v,
                                                      csplit=2 if v == 4 else 0)
    # RexNet instances: 3_1_56 kst 2, 3_2_56 kst 2 and 3, 3_1_28 kst 3 and 4, 3_2_28 kst 3, and the variant-3 one-tile forms
    rex = dict(act_d=ACT_NONE)
    C["sweep_rex_3_2_56_kst3_b9"] = Case("sweep", 9, 56, 56, 80, 88, 3, 2, **rex)                 # 6 tiles, 3 passes, mid % 16 == 8
    C["sweep_rex_3_1_28_kst3_cs2"] = Case("sweep", 3, 28, 28, 80, 96, 3, 1, csplit=2, dup=(0, 2), **rex)
    C["sweep_rex_3_1_28_kst4_b1"] = Case("sweep", 1, 28, 28, 104, 72, 3, 1, **rex)
    C["sweep_rex_3_2_28_kst3_poolnull"] = Case("sweep", 2, 28, 28, 96, 80, 3, 2, pool=False, **rex)
    C["sweep_rex_3_1_56_v3"] = Case("sweep", 2, 56, 56, 48, 56, 3, 1, variant=3, **rex)
    C["sweep_rex_3_2_56_kst2_v3"] = Case("sweep", 2, 56, 56, 64, 48, 3, 2, variant=3, **rex)
    C["sweep_rex_3_2_56_kst3_v3"] = Case("sweep", 1, 56, 56, 72, 40, 3, 2, variant=3, **rex)
    C["sweep_rex_3_1_28_v3_is_default"] = Case("sweep", 2, 28, 28, 80, 32, 3, 1, variant=3, **rex)
    # csplit forced to the B = 256 value on the two-tile RexNet form: 324 -> 328 has 21 tiles, 11 passes (the last holds one tile), 4
    # workgroups walk 3 + 3 + 3 + 2 of them
    C["sweep_rex_54_324_cs4"] = Case("sweep", 2, 56, 56, 56, 328, 3, 1, csplit=4, dup=(0, 1), **rex)
    # the models' own layers (the launch plan golden's sweep steps at 224 x 224); channel counts padded to 8 as the packer does
    for name, (m, cin, mid, k, s, ad) in {
            "eff_24_144": (112, 24, 144, 3, 2, ACT_SILU), "eff_32_192_k3s1": (56, 32, 192, 3, 1, ACT_SILU),
            "eff_32_192_k5s2": (56, 32, 192, 5, 2, ACT_SILU), "eff_48_288_k5s1": (28, 48, 288, 5, 1, ACT_SILU),
            "eff_48_288_k3s2": (28, 48, 288, 3, 2, ACT_SILU),
            "rex150_24_144": (112, 24, 144, 3, 2, ACT_NONE), "rex150_41_246": (56, 48, 248, 3, 1, ACT_NONE),
            "rex150_58_348": (56, 64, 352, 3, 2, ACT_NONE), "rex150_75_450": (28, 80, 456, 3, 1, ACT_NONE),
            "rex150_92_552": (28, 96, 552, 3, 2, ACT_NONE),
            "rex200_32_192": (112, 32, 192, 3, 2, ACT_NONE), "rex200_54_324": (56, 56, 328, 3, 1, ACT_NONE),
            "rex200_77_462": (56, 80, 464, 3, 2, ACT_NONE), "rex200_100_600": (28, 104, 600, 3, 1, ACT_NONE)}.items():
        C[f"sweep_model_{name}_at{m}"] = Case("sweep", 2 if m < 112 else 1, m, m, cin, mid, k, s, act_d=ad)
    return C


CASES = _cases()


# ------------------------------------------------------------------------------------------------------ data (CPU, seeded)
def _bf(t):
    return t.to(torch.bfloat16).float()


class Data:
    """Seeded operands of one case.  x [B][H][W][Cin] and the weights hold bf16 values in fp32; every image has its own scale and
    offset, so a read from the wrong image shows up."""

    def __init__(self, c: Case):
        g = torch.Generator().manual_seed(4000 + c.B * 7 + c.H * 131 + c.W * 17 + c.Cin * 3 + c.mid * 11 + c.k + 5 * c.stride + c.seed)
        b = torch.arange(c.B)
        scale = 0.6 + 0.5 * ((b * 7) % 13).float() / 13 + 0.002 * b.float()
        offset = 0.1 * ((b * 5) % 11).float() / 11
        x = torch.randn(c.B, c.H, c.W, c.Cin, generator=g) * scale[:, None, None, None] + offset[:, None, None, None]
        if c.dup:
            x[c.dup[1]] = x[c.dup[0]]
        self.x = _bf(x)
        self.we = _bf(torch.randn(c.mid, c.Cin, generator=g) / math.sqrt(c.Cin))
        self.be = torch.randn(c.mid, generator=g) * 0.3
        self.wd = _bf(torch.randn(c.k * c.k, c.mid, generator=g) * (1.5 / c.k))       # [k*k][mid], tap ky * k + kx
        self.bd = torch.randn(c.mid, generator=g) * 0.2

    def we_packed(self, c: Case):
        """[ceil16(mid)][ceil32(Cin)] zero padded (GEMM packing), and the bias [ceil16(mid)]"""
        w = torch.zeros((c.mid + 15) // 16 * 16, kpad32(c.Cin))
        w[:c.mid, :c.Cin] = self.we
        b = torch.zeros(w.shape[0])
        b[:c.mid] = self.be
        return w, b


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


def ulp_bf16(v):
    """spacing of the bf16 numbers around the float64 values v (8 significant bits; normal range)"""
    _, e = np.frexp(v.numpy())
    return torch.from_numpy(np.ldexp(1.0, e - 8))


def round_bf16(v):
    """float64 -> nearest bf16 value, ties to even, computed on the float64 value itself"""
    u = ulp_bf16(v)
    return torch.from_numpy(np.rint((v / u).numpy())) * u


def midpoint_distance(v):
    """distance of the float64 values v from the nearest midpoint between two bf16 neighbours"""
    u = ulp_bf16(v)
    q = v / u
    return ((q - torch.floor(q)) - 0.5).abs() * u


def _taps(e, wd, c: Case, pad_mode="zero", pad_rows=None):
    """sum over taps of e[b][oy s - k/2 + ky][ox s - k/2 + kx][n] wd[ky k + kx][n]; e [B][H][W][mid] float64 -> [B][Ho][Wo][mid].
    pad_mode "edge": replicate padding; pad_rows [mid]: value of the rows outside the image (the columns stay zero)."""
    k, s, p = c.k, c.stride, c.k // 2
    B, H, W, M = e.shape
    if pad_mode == "edge":
        ep = torch.nn.functional.pad(e.permute(0, 3, 1, 2), (p, p, p, p), mode="replicate").permute(0, 2, 3, 1)
    else:
        ep = torch.zeros(B, H + 2 * p, W + 2 * p, M, dtype=e.dtype)
        if pad_rows is not None:
            ep[:, :p, p:p + W] = pad_rows
            ep[:, p + H:, p:p + W] = pad_rows
        ep[:, p:p + H, p:p + W] = e
    out = torch.zeros(B, c.Ho, c.Wo, M, dtype=e.dtype)
    for ky in range(k):
        for kx in range(k):
            out += ep[:, ky:ky + (c.Ho - 1) * s + 1:s, kx:kx + (c.Wo - 1) * s + 1:s] * wd[ky * k + kx]
    return out


def squeeze_mask(c: Case, what):
    """[Ho][Wo] float64, 0 on the pixels of the last depthwise strip of every row ("strip": late and band kernels, PX pixels per thread)
    or of the last row band ("band": band and sweep kernels)."""
    m = torch.ones(c.Ho, c.Wo, dtype=torch.float64)
    if what == "strip":
        px = _px(c.W, c.k, c.stride)
        m[:, (cdiv(c.Wo, px) - 1) * px:] = 0.0
    else:
        m[(cdiv(c.Ho, c.TH) - 1) * c.TH:] = 0.0
    return m


MUTANTS = {
    "pad_reads_edge": lambda c: True,
    "halo_rows_hold_act_of_bias": lambda c: True,
    "squeeze_misses_last_strip": lambda c: c.pool and c.family != "sweep",
    "squeeze_misses_last_band": lambda c: c.pool and c.family != "late" and c.TH < c.Ho,
    "partial_slab_group_from_slab0": lambda c: c.mid % c.slab != 0 and c.mid > c.slab,
    "stride2_phase_shifted": lambda c: c.stride == 2,
    "taps_transposed": lambda c: True,
    "e_left_unrounded": lambda c: True,
    "expand_drops_later_ksteps": lambda c: c.Cin > 32,
    "image_reads_previous_image": lambda c: c.B > 1 and c.dup != (0, 1),
}


def reference(c: Case, d: Data, mutant=None):
    """{"D": (ref [B][Ho][Wo][mid], tol), "pool": (ref [B][mid] mean over pixels, tol)} float64 and the flippable share of E.
    `mutant` names a deliberate bug (test_mutants_are_far_outside_the_tolerance); tolerances are then not computed."""
    x, we, be = d.x.double(), d.we.double(), d.be.double()
    wd, bd = d.wd.double(), d.bd.double()
    if mutant == "expand_drops_later_ksteps":
        we = we.clone()
        we[:, 32:] = 0.0
    if mutant == "image_reads_previous_image":
        x = torch.cat([x[:1], x[:-1]])
    if mutant == "taps_transposed":
        wd = wd.view(c.k, c.k, c.mid).transpose(0, 1).reshape(c.k * c.k, c.mid)
    e64 = _act(x @ we.t() + be, c.act_e)
    e_r = e64 if mutant == "e_left_unrounded" else round_bf16(e64)
    if mutant == "stride2_phase_shifted":
        e_r = torch.cat([e_r[:, :, 1:], torch.zeros_like(e_r[:, :, :1])], dim=2)
    if mutant == "pad_reads_edge":
        t = _taps(e_r, wd, c, pad_mode="edge")
    elif mutant == "halo_rows_hold_act_of_bias":
        t = _taps(e_r, wd, c, pad_rows=round_bf16(_act(be, c.act_e)))
    else:
        t = _taps(e_r, wd, c)
    v = _act(t + bd, c.act_d)
    if mutant == "partial_slab_group_from_slab0":
        v = v.clone()
        v[..., c.mid - 8:] = v[..., (c.mid - 8) % c.slab:(c.mid - 8) % c.slab + 8]
    vs = v
    if mutant == "squeeze_misses_last_strip":
        vs = v * squeeze_mask(c, "strip")[None, :, :, None]
    if mutant == "squeeze_misses_last_band":
        vs = v * squeeze_mask(c, "band")[None, :, :, None]
    pool = vs.mean((1, 2))
    if mutant is not None:
        return {"D": (v, None), "pool": (pool, None)}, None
    magE = DERIV[c.act_e] * (x.abs() @ we.abs().t() + be.abs())
    flippable = midpoint_distance(e64) <= TOL_E * magE
    slack = torch.where(flippable, ulp_bf16(e64), torch.zeros_like(e64))
    magD = DERIV[c.act_d] * (_taps(e_r.abs(), wd.abs(), c) + bd.abs())
    slackD = DERIV[c.act_d] * _taps(slack, wd.abs(), c)
    res = {"D": (v, TOL_REL * v.abs() + TOL_DW * magD + slackD),
           "pool": (pool, TOL_DW * magD.mean((1, 2)) + slackD.mean((1, 2)))}
    return res, flippable.double().mean().item()
