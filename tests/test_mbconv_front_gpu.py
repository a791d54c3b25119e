"""The fused expand + depthwise kernels, every template instance, elementwise against float64.

k_fused_late and k_fused_band (csrc/fused_mbconv.hip) and k_sweep_mbconv (csrc/sweep_mbconv.hip) run the expand and depthwise
convs of every MBConv / RexNet block from 112x112 down to 7x7.  The model reaches them only inside whole blocks, checked by a
relative L2 bound that a wrong last strip, last band, halo row or pad column (a few pixels out of thousands) cannot move.  Here
each case is ONE call of the developer entry mi355_mbconv_front_ex.  The call reports the instantiation that ran
(MI355_FRONT_PATH_*), and the test asserts first that it is the one the case is named for: 24 late, 32 band and 58 sweep
instances, enumerated from the launchers' rules in tests/mbconv_front_ref.py, each have a case.  Then D and the squeeze sums are
compared elementwise with the float64 reference and the tolerance of tests/mbconv_front_ref.py (its docstring derives them).
D and pool are pre-filled with NaN and followed by a NaN guard, so an unwritten element or an overrun shows up; every image has
its own scale and offset; where a case names a repeated image, the two copies must come out with identical bits although they
sit at different batch positions (different slab rotation, different workgroup).

The functions without the gpu marker check the tests themselves on the CPU: the cases cover every reachable instance, the
flippable share of each case's E elements stays at or below 5 %, and ten deliberate bugs applied to the reference (edge padding,
halo rows holding act(bias), the squeeze missing its last strip or band, a partial slab's last channel group taken from slab 0,
a shifted stride-2 phase, transposed taps, E left un-rounded, the expand dropping its later k-steps, an image reading its
neighbour's input) each move some output more than 10x its tolerance on each case's own data.

Worst |err| / tol per family as measured on the MI355X (every case of the family; printed by the test):
    late   D 0.994   squeeze 0.631
    band   D 0.994   squeeze 0.951
    sweep  D 0.995   squeeze 0.724
D comes close to 1 by construction: half an ulp of the bf16 output is up to 2^-8 |ref|, the tolerance's first term.  The squeeze
comes close where most of a channel's few flippable E elements did flip (small maps: each flip uses up its whole slack).

Found by these cases: k_sweep_mbconv<5, 2, 56, TH = 1> (sweep_variant 4 of class 5_2_56, a tuning instance) has a halo of three rows
and two new rows per band, so band -1 left buffer row 2 - band 0's row above the image - to whatever the previous slab of the
same workgroup had put there: row 0 of D was wrong in every slab but a workgroup's first (|err| / tol 36497 in
sweep_5_2_56_variant4, which forces two slabs per workgroup).  The kernel now zeroes those rows at the start of each slab."""
import ctypes
import json
import os
import re

import pytest
import torch

from helpers import ROOT
from mbconv_front_ref import (ACT_INST, ACT_NONE, ACT_SILU, CASES, FLIP_CAP, GUARD, KERNELS, MARGIN, MUTANTS, SWEEP_CLASS, Case, Data,
                              auto_family, reachable_instances, reference, round_bf16, squeeze_mask)

DEV = "cuda:0"
_REF = {}                   # name -> (Data, reference, flippable share): computed once, shared, never changed


def ref_of(name):
    if name not in _REF:
        d = Data(CASES[name])
        _REF[name] = (d,) + reference(CASES[name], d)
    return _REF[name]


# -------------------------------------------------------------------------------------------------------------------- CPU
def test_every_dispatch_branch_has_a_case():
    want = reachable_instances()
    assert len([t for t in want if t[0] == "late"]) == 24
    assert len([t for t in want if t[0] == "band"]) == 32
    assert len([t for t in want if t[0] == "sweep"]) == 58
    assert not any(t[0] == "band" and t[5] == 96 for t in want), "band_slab() never selects a 96-channel slab"
    got = {c.instance for c in CASES.values()}
    assert want <= got, sorted(want - got)
    assert got <= want, sorted(got - want)
    cs = list(CASES.values())
    for name, c in CASES.items():
        assert c.supported, name
        assert not c.dup or c.dup[1] < c.B, name
    late = [c for c in cs if c.family == "late"]
    assert any(c.Cin == 8 for c in late) and any(c.Cin % 32 for c in late) and any(c.mid % 16 == 8 for c in late)
    for niw in (4, 2, 1):
        assert any(c.mid == 128 * niw + 8 and c.instance[3] == niw for c in late), niw
    assert any(c.Wo % c.instance[4] for c in late), "a partial last strip"
    # B = 100: two workgroups per image with 2 + 1 slabs; B = 130: one workgroup, three slabs, more images than slabs
    assert any(c.B == 100 and -(-c.mid // c.slab) == 3 and c.dup for c in late)
    assert any(c.B == 130 and -(-c.mid // c.slab) == 3 and c.mid % c.slab == 8 and c.dup for c in late)
    band = [c for c in cs if c.family == "band"]
    assert any(c.mid % 64 and c.mid % 48 for c in band), "a partial last slab"
    assert {1, 0} <= {c.band_rows for c in band} and any(c.Ho % c.TH for c in band)
    assert any(c.W == 128 for c in band) and any(c.nblk > 2 for c in band)
    sweep = [c for c in cs if c.family == "sweep"]
    for m, b256 in ((112, 3), (56, 4), (28, 2)):
        at = [c for c in sweep if c.W == m]
        assert any(c.B == 1 for c in at) and any(c.B == 9 for c in at) and any(not c.pool for c in at), m
        assert any(c.mid % 16 == 8 for c in at), m
        # several slabs per workgroup from an image-dependent start, with the split of B = 256
        assert any(c.csplit == b256 and -(-c.mid // c.slab) >= 2 * b256 and c.dup for c in at), m
        assert any(c.csplit and -(-c.mid // c.slab) % c.used_csplit for c in at), m
    assert any(c.sweep["ns"] == 2 and -(-c.mid // 16) % 2 for c in sweep), "an odd tile count with two tiles per pass"
    for mut, applies in MUTANTS.items():
        for fam in ("late", "band", "sweep"):
            if (mut, fam) not in {("squeeze_misses_last_strip", "sweep"), ("squeeze_misses_last_band", "late")}:
                assert any(applies(c) for c in cs if c.family == fam), (mut, fam)


def test_path_enum_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"MI355_FRONT_KERNEL_([A-Z]+)\s*=\s*(\d+)", txt)}
    assert got == KERNELS
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"MI355_FRONT_ACT_([A-Z_]+)\s*=\s*(\d+)", txt)}
    assert got == ACT_INST
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"MI355_SWEEP_CLASS_([0-9_]+)\s*=\s*(\d+)", txt)}
    assert got == SWEEP_CLASS
    # the sweep kernel's own class numbers are the header's, in the launcher's order
    src = open(os.path.join(ROOT, "imageretrievalresearch_amd", "csrc", "sweep_mbconv.hip")).read()
    order = re.search(r"enum \{ SW_NONE = 0, ([^}]*)\};", src).group(1).replace("SW_", "").replace(" ", "").split(",")
    assert {n: i + 1 for i, n in enumerate(order)} == SWEEP_CLASS

    def shifts(macro):
        body = re.search(r"#define " + macro + r"\((?:[^\n]*\\\n)*[^\n]*", txt).group(0)
        return dict(re.findall(r"\((\w+)\) << (\d+)", body))
    assert "((ks) == 5) << 2 | ((s) == 2) << 3" in txt
    assert shifts("MI355_FRONT_PATH_LATE") == {"niw": "4", "px": "8"}
    assert shifts("MI355_FRONT_PATH_BAND") == {"kst": "4", "px": "8", "mc": "12", "th": "20"}
    assert shifts("MI355_FRONT_PATH_SWEEP") == {"cls": "4", "kst": "8", "ns": "12", "variant": "14", "act": "17", "csplit": "19"}


def test_band_kernel_has_no_96_channel_slab():
    src = open(os.path.join(ROOT, "imageretrievalresearch_amd", "csrc", "fused_mbconv.hip")).read()
    assert "96>" not in src and "% 96" not in src


def test_bf16_rounding_of_float64_values():
    """round_bf16 rounds the float64 value itself: equal to torch's conversion on fp32-exact inputs, ties to even, and right where
    a detour through float32 is wrong (a value just above a midpoint that float32 rounds onto the midpoint)."""
    g = torch.Generator().manual_seed(5)
    v = (torch.randn(20000, generator=g) * torch.logspace(-6, 6, 20000)).double()
    assert torch.equal(round_bf16(v), v.float().to(torch.bfloat16).double())
    tie = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)], dtype=torch.float64)
    assert round_bf16(tie).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]
    above = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert round_bf16(above).item() == 1.0 + 2.0 ** -7
    assert above.float().to(torch.bfloat16).item() == 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_mutants_are_far_outside_the_tolerance(name):
    """CPU only, on this case's data: at most FLIP_CAP of the E elements are flippable, and each applicable bug moves some D or
    squeeze value more than MARGIN x its tolerance."""
    c = CASES[name]
    d, ref, share = ref_of(name)
    print(f"front {name}: flippable share of E {100 * share:.2f} %")
    assert share <= FLIP_CAP, f"{name}: {100 * share:.2f} % of the E elements are flippable"
    for mut, applies in MUTANTS.items():
        if not applies(c):
            continue
        m, _ = reference(c, d, mut)
        keys = ("D", "pool") if c.pool else ("D",)
        ratio = max(((m[k][0] - ref[k][0]).abs() / ref[k][1]).max().item() for k in keys)
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


def test_squeeze_masks_cover_a_real_last_piece():
    for name, c in CASES.items():
        if MUTANTS["squeeze_misses_last_strip"](c):
            assert int((squeeze_mask(c, "strip") == 0).sum()) > 0, name
        if MUTANTS["squeeze_misses_last_band"](c):
            m = squeeze_mask(c, "band")
            assert 0 < int((m == 0).sum()) < m.numel(), name


# ------------------------------------------------------------------------------------------------------------------- GPU
def _run(c: Case, d: Data, kernel=None):
    """One call of mi355_mbconv_front_ex -> (path, pool_nblk, D [B][Ho][Wo][mid], pool [B][nblk][mid] or None, guards)."""
    from imageretrievalresearch_amd._lib import MbconvFrontArgs, check, lib, stream_ptr
    we, be = d.we_packed(c)
    x = d.x.to(torch.bfloat16).to(DEV).contiguous()
    we, wd = we.to(torch.bfloat16).to(DEV), d.wd.to(torch.bfloat16).to(DEV).contiguous()
    be, bd = be.to(DEV), d.bd.to(DEV)
    nD, nP = c.B * c.Ho * c.Wo * c.mid, c.B * c.nblk * c.mid
    D = torch.full((nD + GUARD,), float("nan"), device=DEV, dtype=torch.bfloat16)
    P = torch.full((nP + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    a = MbconvFrontArgs(X=x.data_ptr(), We=we.data_ptr(), be=be.data_ptr(), Wd=wd.data_ptr(), bd=bd.data_ptr(), D=D.data_ptr(),
                        pool=P.data_ptr() if c.pool else None, B=c.B, H=c.H, W=c.W, Cin=c.Cin, mid=c.mid, k=c.k, stride=c.stride,
                        act_e=c.act_e, act_d=c.act_d, kernel=KERNELS[kernel or c.kernel], band_rows=c.band_rows,
                        sweep_variant=c.variant, sweep_csplit=c.csplit)
    path, nblk = ctypes.c_int(-1), ctypes.c_int(-1)
    check(lib().mi355_mbconv_front_ex(ctypes.byref(a), ctypes.byref(nblk), ctypes.byref(path), stream_ptr(DEV)))
    torch.cuda.synchronize()
    Dh, Ph = D.cpu(), P.cpu()
    return (path.value, nblk.value, Dh[:nD].view(c.B, c.Ho, c.Wo, c.mid), Ph[:nP].view(c.B, c.nblk, c.mid) if c.pool else None,
            {"D": Dh[nD:], "pool": Ph[nP:]})


def _worst(got, ref, tol):
    ratio = (got - ref).abs() / tol
    i = int(ratio.argmax())
    return ratio.view(-1)[i].item(), tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ratio.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_front_half_matches_float64(name):
    c = CASES[name]
    d, ref, share = ref_of(name)
    path, nblk, D, pool, guards = _run(c, d)
    assert path == c.code, f"{name}: ran path {path:#x}, expected {c.code:#x} = {c.instance} TH {c.TH}"
    assert nblk == c.nblk, (name, nblk, c.nblk)
    for k, g in guards.items():
        assert torch.isnan(g).all(), f"{name}: wrote past the end of {k}"
    bad = torch.isnan(D.float()).nonzero()
    assert bad.numel() == 0, f"{name}: D unwritten at (image, y, x, channel) {bad[0].tolist()}"
    wD, at = _worst(D.double(), *ref["D"])
    msg = f"front {name:44s} {c.family:5s} {str(c.instance[1:]):24s} flippable {100 * share:.2f} %: worst |err| / tol D {wD:.3f}"
    assert wD <= 1.0, f"{name} {c.instance}: D |err| / tol {wD:.3f} at (image, y, x, channel) {at}"
    if c.pool:
        bad = torch.isnan(pool).nonzero()
        assert bad.numel() == 0, f"{name}: pool unwritten at (image, block, channel) {bad[0].tolist()}"
        wP, at = _worst(pool.double().sum(1) / (c.Ho * c.Wo), *ref["pool"])
        msg += f" squeeze {wP:.3f}"
        assert wP <= 1.0, f"{name} {c.instance}: squeeze |err| / tol {wP:.3f} at (image, channel) {at}"
    else:
        assert torch.isnan(guards["pool"]).all() and nblk == 1
    if c.dup:
        i, j = c.dup
        assert torch.equal(D[i].view(torch.int16), D[j].view(torch.int16)), f"{name}: images {i} and {j} hold the same input, D differs"
        assert not c.pool or torch.equal(pool[i], pool[j]), f"{name}: images {i} and {j} hold the same input, the squeeze differs"
    print(msg)


def golden_front_layers():
    """[(model, Case with kernel "auto", family or None)]: every expand + depthwise pair of the three convolutional backbones at
    224 x 224 with what the committed launch-plan golden records for it under default options (batch 1: no whole-block kernel)."""
    from launch_plan_cases import decode_steps
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")))
    L, out = g["lists"], []
    for model in ("efficientnet_b3a", "rexnet_150", "rexnet_200"):
        first_op, n_ops, how = decode_steps(L[g["plans"][f"{model}|1|1|224x224|defaults|features"][0]])
        labels = L[g["profile_ops"][f"{model}|1|224x224"][0]]
        seen = set()
        for f, n, h in zip(first_op, n_ops, how):
            a = re.match(r"pw (\d+)->(\d+) @(\d+)x(\d+)$", labels[f])
            b = re.match(r"dw k(\d) s(\d) C(\d+)", labels[f + 1]) if a and f + 1 < len(labels) else None
            if not b or (a.groups(), b.groups()) in seen:
                continue
            seen.add((a.groups(), b.groups()))
            fam = {"fused_late": "late", "sweep": "sweep", "band": "band", "op": None}[g["how"][h]]
            assert (n == 2) == (fam is not None)
            cin, mid, H, W = (int(v) for v in a.groups())
            c = Case("auto", 1, H, W, (cin + 7) & ~7, (mid + 7) & ~7, int(b.group(1)), int(b.group(2)),
                     act_d=ACT_SILU if model.startswith("eff") else ACT_NONE)
            out.append((model, c, fam))
    return out


def test_auto_rule_agrees_with_the_launch_plan_golden():
    """CPU: the launchers' rules as written out in mbconv_front_ref.py give the family the golden records, layer by layer."""
    layers = golden_front_layers()
    assert len(layers) >= 40 and {f for _, _, f in layers} == {"late", "sweep", None}
    for model, c, fam in layers:
        assert auto_family(c.H, c.W, c.Cin, c.mid, c.k, c.stride, c.act_e, c.act_d) == fam, (model, c)


@pytest.mark.gpu
def test_auto_takes_the_launch_plans_decision():
    """kernel AUTO reports, for every front-half layer of the three backbones at 224 x 224, the family the committed launch-plan
    golden records for it, and refuses the layers the plan runs unfused."""
    from imageretrievalresearch_amd._lib import lib
    for model, c, fam in golden_front_layers():
        d = Data(c)
        if fam is None:
            with pytest.raises(RuntimeError, match="unfused"):
                _run(c, d)
            continue
        path, nblk, D, pool, guards = _run(c, d)
        assert path == c.code and path & 3 == KERNELS[fam], (model, c, hex(path))
        assert not torch.isnan(D.float()).any() and torch.isnan(guards["D"]).all(), (model, c)
    assert lib().mi355_abi_version() == 3
