"""The whole-block MBConv kernel, every template instance, elementwise against float64.

k_mbconv_block (csrc/mbconv_block.hip) runs every 14x14 and 7x7 MBConv / RexNet block in one launch once the batch reaches 96
images: expand, depthwise, SE squeeze, two FCs, sigmoid, gated projection and residual.  The models reach it only inside whole
networks or whole blocks, checked by a relative L2 bound over a whole tensor that a wrong last pixel row, a wrong last 8 channels of
a slab, a dropped hidden unit, a gate chunk from the neighbouring image or a residual past res_n cannot move.  Here each case is ONE
call of the developer entry mi355_mbconv_block_ex.  The call reports the instantiation that ran and the launcher's run-time choices
(MI355_BLOCK_PATH), and the test asserts first that they are what the launcher's rules, written out in tests/mbconv_block_ref.py,
predict for the case.  Then the kernel's depthwise output D and the block output Y are compared elementwise with the float64
reference and the staged tolerance of tests/mbconv_block_ref.py (its docstring derives them).  D and Y are pre-filled with NaN
and followed by a NaN guard; every image has its own scale.  One case per instance is also run with eleven copies of one image,
more than any rotation period: every batch position must give the same bits, with and without the rotations (norot 0 / 15).

The functions without the gpu marker check the tests themselves on the CPU: the cases cover all 18 instances, every block shape
the three models' plans run whole-block at 224 x 224 and every listed edge in a SiLU and a linear-depthwise instance; the Python
copy of the launcher's rules agrees with mi355_mbconv_block_how on a few thousand shapes; the flippable shares of each case's E
and A' elements stay at or below 5 %; and fifteen deliberate bugs applied to the reference each move some element of D or Y more
than 10x its tolerance on every case they apply to.

Worst |err| / tol per instance family as measured on the MI355X (every case of the family; printed by the test):
    14x14 SiLU    D 0.995   Y 0.994        7x7 SiLU    D 0.995   Y 0.992
    14x14 linear  D 0.995   Y 0.995        7x7 linear  D 0.995   Y 0.995
Both come close to 1 by construction: half an ulp of a bf16 output is up to 2^-8 |ref|, the tolerance's first term.  Flippable
shares: E 0.00 ... 0.17 %, A' 0.04 ... 1.38 %.  No case failed; the non-square maps the support check accepts do work."""
import ctypes
import json
import os
import re

import pytest
import torch

from helpers import ROOT
from mbconv_block_ref import (ACT_NONE, ACT_RELU, ACT_SILU, CASES, FLIP_CAP, GUARD, INSTANCES, MARGIN, MODEL_LAYERS, MUTANTS, ROT_B, TERMS,
                              Case, Data, block_how, block_path, front, mutant_outputs, pad8, path_fields, rotation_cases, tail)

DEV = "cuda:0"
_REF = {}                   # name -> (Data, Front): computed once, shared, never changed


def ref_of(name):
    if name not in _REF:
        d = Data(CASES[name])
        _REF[name] = (d, front(CASES[name], d))
    return _REF[name]


def family(c: Case):
    return f"{c.W}x{c.W} {'SiLU' if c.act_d == ACT_SILU else 'linear'}"


# -------------------------------------------------------------------------------------------------------------------- CPU
def test_every_instance_model_layer_and_edge_has_a_case():
    cs = list(CASES.values())
    for name, c in CASES.items():
        assert c.supported, name
        assert c.B == 3 and not c.same, name
        assert c.res_n == 0 or (c.stride == 1 and c.res_n % 8 == 0 and 8 <= c.res_n <= min(c.Cin, c.Cout)), name
    assert len(INSTANCES) == 18 and len(set(INSTANCES)) == 18
    got = {c.instance for c in cs}
    assert got == set(INSTANCES), sorted(set(INSTANCES) ^ got)
    print("\ninstance (k, stride, W, KST, NTW, act_d): cases")
    for t in INSTANCES:
        print(f"    {str(t):24s} {sum(c.instance == t for c in cs)}")
    # every whole-block shape of the three models
    assert len([c for c in cs if c.model]) == len(MODEL_LAYERS) == 23
    edges = {
        "mid 8": lambda c: c.mid == 8,
        "mid 120 (one slab, an idle wave)": lambda c: c.mid == 120,
        "mid 128 (one slab, no idle wave)": lambda c: c.mid == 128,
        "mid 136 (second slab, one active wave)": lambda c: c.mid == 136,
        "mid 264": lambda c: c.mid == 264,
        "mid % 16 == 8": lambda c: c.mid % 16 == 8 and c.mid > 136,
        "mid of the 1392 class": lambda c: 1392 <= c.mid <= 1400,
        "mid of the 2304 class": lambda c: 2056 <= c.mid <= 2304,
        "mid 2560 (the largest)": lambda c: c.mid == 2560,
        "Cin % 32 == 0": lambda c: c.Cin % 32 == 0, "Cin % 32 == 8": lambda c: c.Cin % 32 == 8, "Cin % 32 == 24": lambda c: c.Cin % 32 == 24,
        "Cout % 16 == 8": lambda c: c.Cout % 16 == 8,
        "rd 1": lambda c: c.rd == 1, "rd 3": lambda c: c.rd == 3, "rd 4": lambda c: c.rd == 4, "rd 5": lambda c: c.rd == 5,
        "rd 16 JS": lambda c: c.rd == 16 * c.f["js"], "rd 16 JS + 1": lambda c: c.rd == 16 * c.f["js"] + 1,
        "rd 173": lambda c: c.rd == 173, "rd 192": lambda c: c.rd == 192,
        "JS 8": lambda c: c.f["js"] == 8, "JS 2": lambda c: c.f["js"] == 2, "JS 1": lambda c: c.f["js"] == 1,
        "rd 16 JS and 16 JS + 1 with JS 8": lambda c: c.f["js"] == 8 and c.rd in (128, 129),
        "rd 16 JS and 16 JS + 1 with JS 2": lambda c: c.f["js"] == 2 and c.rd in (32, 33),
        "rd 16 JS and 16 JS + 1 with JS 1": lambda c: c.f["js"] == 1 and c.rd in (16, 17),
        "map 7x7": lambda c: (c.H, c.W) == (7, 7), "map 14x14": lambda c: (c.H, c.W) == (14, 14),
        "map 5x7": lambda c: (c.H, c.W) == (5, 7), "map 9x7": lambda c: (c.H, c.W) == (9, 7),
        "map 10x14": lambda c: (c.H, c.W) == (10, 14), "map 13x14": lambda c: (c.H, c.W) == (13, 14),
        "non-square map with the counted wait (8x7)": lambda c: not c.square and c.counted_wait,
        "non-square map draining (vmcnt 0)": lambda c: not c.square and not c.counted_wait,
        "residual none": lambda c: c.res_n == 0, "residual on every column": lambda c: c.res_n == c.Cout,
        "residual on a part": lambda c: 0 < c.res_n < c.Cout,
        "ReLU6 behind the gate": lambda c: c.a_relu6 == 1, "no ReLU6": lambda c: c.a_relu6 == 0,
        "SE SiLU": lambda c: c.se_act == ACT_SILU, "SE ReLU": lambda c: c.se_act == ACT_RELU,
        "X rows wide": lambda c: c.f["xwide"] == 1, "X rows compact": lambda c: c.f["xwide"] == 0,
        "X rows compact, Cin % 32 != 0": lambda c: c.f["xwide"] == 0 and c.Cin % 32 != 0,
        "projection whole, 1 super-chunk": lambda c: c.f["whole"] and c.f["nsc"] == 1,
        "projection whole, 2 super-chunks": lambda c: c.f["whole"] and c.f["nsc"] == 2,
        "projection whole, >= 3 super-chunks": lambda c: c.f["whole"] and c.f["nsc"] >= 3,
        "projection chunked, 1 chunk": lambda c: not c.f["whole"] and c.nchunks == 1,
        "projection chunked, 2 chunks": lambda c: not c.f["whole"] and c.nchunks == 2,
        "projection chunked, >= 3 chunks": lambda c: not c.f["whole"] and c.nchunks >= 3,
    }
    print("edge: cases on SiLU-depthwise / on linear-depthwise instances")
    for what, has in edges.items():
        n = [sum(1 for c in cs if c.act_d == ad and has(c)) for ad in (ACT_SILU, ACT_NONE)]
        print(f"    {what:48s} {n[0]:3d} / {n[1]:3d}")
        assert n[0] > 0 and n[1] > 0, what
    # what only one family's instances allow
    only = {
        "stride 2 from 14x14 (SiLU only)": lambda c: c.stride == 2 and (c.H, c.W) == (14, 14),
        "stride 2 from 10x14 (SiLU only)": lambda c: c.stride == 2 and (c.H, c.W) == (10, 14),
        "stride 2 from 13x14 (SiLU only)": lambda c: c.stride == 2 and (c.H, c.W) == (13, 14),
        "NTW 4 (linear only)": lambda c: c.f["ntw"] == 4,
    }
    for what, has in only.items():
        print(f"    {what:48s} {sum(1 for c in cs if has(c)):3d}")
        assert any(has(c) for c in cs), what
    # NTW flips on one instance family (k, stride, W, KST, act_d) between neighbouring widths: 2 <-> 3 at 14x14 and 7x7, 3 <-> 4
    flips = {(c.instance[:4] + (c.act_d,), c.Cout): c.f["ntw"] for c in cs if c.mid == 264 and c.square}
    for key, lo, hi, a, b in (((3, 1, 14, 4, ACT_NONE), 96, 104, 3, 2), ((3, 1, 14, 4, ACT_NONE), 128, 136, 2, 3),
                              ((3, 1, 14, 6, ACT_NONE), 192, 200, 3, 4), ((3, 1, 7, 8, ACT_NONE), 48, 56, 2, 3),
                              ((3, 1, 7, 8, ACT_NONE), 192, 200, 3, 2), ((3, 1, 7, 8, ACT_NONE), 256, 264, 2, 3)):
        assert (flips[key, lo], flips[key, hi]) == (a, b), (key, lo, hi)
    # the batch-position cases: one per instance, more images than any rotation period, and the rotations do something
    rot = rotation_cases()
    assert {c.instance for c in rot.values()} == set(INSTANCES) and len(rot) == 18
    for name, c in rot.items():
        assert c.B == ROT_B and c.same
        assert 1 < c.nslabs < ROT_B and 1 < c.ngroups < ROT_B and 1 < c.nwn < ROT_B, (name, c.nslabs, c.ngroups, c.nwn)
    for mut, applies in MUTANTS.items():
        for ad in (ACT_SILU, ACT_NONE):
            if (mut, ad) != ("squeeze_divided_by_input_hw", ACT_NONE):         # no linear-depthwise instance has stride 2
                assert any(applies(c) for c in cs if c.act_d == ad), (mut, ad)
    assert len(MUTANTS) >= 10


def test_path_macro_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    body = re.search(r"#define MI355_BLOCK_PATH\((?:[^\n]*\\\n)*[^\n]*", txt).group(0)
    assert re.match(r"#define MI355_BLOCK_PATH\(ks, s, wi, kst, ntw, act_d, xwide, whole, nsc, js\)", body)
    assert dict(re.findall(r"\(\((\w+)\) (?:==|!=) \d+\) << (\d+)", body)) == {"s": "1", "wi": "2", "xwide": "13", "whole": "14"}
    assert "((ks) == 5)" in body and "((s) == 2)" in body and "((wi) == 14)" in body
    assert dict(re.findall(r"\| \((\w+)\) << (\d+)", body)) == {"kst": "3", "ntw": "7", "act_d": "10", "nsc": "15", "js": "20"}
    acc = dict(re.findall(r"#define MI355_BLOCK_PATH_(\w+)\(p\) (.*)", txt))
    assert set(acc) == {"KS", "S", "WI", "KST", "NTW", "ACT_D", "XWIDE", "WHOLE", "NSC", "JS"}
    p = block_path(5, 2, 14, 12, 4, 5, 1, 1, 20, 8)
    want = dict(ks=5, s=2, wi=14, kst=12, ntw=4, act_d=5, xwide=1, whole=1, nsc=20, js=8)
    assert path_fields(p) == want
    for name, expr in acc.items():                                        # each accessor: a shift, a mask, two of them a choice
        sh, mask = re.search(r">> (\d+)", expr), re.search(r"& (\d+)", expr)
        v = p >> (int(sh.group(1)) if sh else 0) & int(mask.group(1))
        pick = re.search(r"\? (\d+) : (\d+)", expr)
        assert (int(pick.group(1 if v else 2)) if pick else v) == want[name.lower()], (name, expr)
    p = block_path(3, 1, 7, 3, 2, 0, 0, 0, 1, 1)
    assert path_fields(p) == dict(ks=3, s=1, wi=7, kst=3, ntw=2, act_d=0, xwide=0, whole=0, nsc=1, js=1)
    # the instance list is the kernel file's
    src = open(os.path.join(ROOT, "imageretrievalresearch_amd", "csrc", "mbconv_block.hip")).read()
    inst = re.search(r"#define MB_INSTANCES\(X\)(.*?)\nstatic bool", src, re.S).group(1)
    acts = {"ACT_SILU": ACT_SILU, "ACT_NONE": ACT_NONE}
    got = [tuple(int(v) for v in m[:5]) + (acts[m[5]],) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+), (\w+)\)", inst)]
    assert got == INSTANCES


def _how(shape):
    from imageretrievalresearch_amd._lib import lib
    p = ctypes.c_int(-1)
    e = lib().mi355_mbconv_block_how(*shape, ctypes.byref(p))
    if e:
        assert p.value == 0 and b"unsupported" in lib().mi355_last_error(), (shape, lib().mi355_last_error())
        return None
    return p.value


def test_python_rules_agree_with_the_launcher():
    """mi355_mbconv_block_how (no device is touched) against the rules written out in mbconv_block_ref.py: supported or not,
    and the path, for every case and on a grid of shapes round every limit of the support check."""
    for name, c in CASES.items():
        assert _how(c.shape) == c.code is not None, name
    n = sup = 0
    for H, W in ((7, 7), (5, 7), (9, 7), (10, 7), (8, 7), (14, 14), (10, 14), (13, 14), (15, 14), (2, 14), (14, 7), (1, 7)):
        for k, s in ((3, 1), (5, 1), (3, 2), (5, 2)):
            for cin in (8, 96, 136, 152, 160, 192, 232, 256, 352, 384):
                for mid in (8, 136, 1392, 2304, 2560, 2568):
                    for cout in (8, 24, 40, 104, 136, 200, 264, 392, 520):
                        for ad in (ACT_NONE, ACT_SILU):
                            shape = (H, W, cin, mid, cout, k, s, 24, ACT_SILU, ad)
                            want = block_how(*shape)
                            assert _how(shape) == want, shape
                            n, sup = n + 1, sup + (want is not None)
    for rd, ae, ok in ((0, ACT_SILU, False), (1, ACT_SILU, True), (192, ACT_SILU, True), (193, ACT_SILU, False), (24, ACT_NONE, False),
                       (24, ACT_RELU, False)):
        shape = (7, 7, 232, 1392, 232, 5, 1, rd, ae, ACT_SILU)
        if rd:
            assert (_how(shape) is not None) == ok == (block_how(*shape) is not None), shape
    print(f"\n{n} shapes, {sup} of them supported")
    assert n > 4000 and sup > 300


@pytest.mark.parametrize("name", list(CASES))
def test_mutants_are_far_outside_the_tolerance(name):
    """CPU only, on this case's data: at most FLIP_CAP of the E elements and of the A' elements are flippable, and each applicable
    bug moves some element of D or Y more than MARGIN x its tolerance (Y's reference taken, as on the GPU, from the D the buggy
    kernel wrote)."""
    c = CASES[name]
    d, fr = ref_of(name)
    t = tail(c, d, fr, mutant_outputs(c, d, fr, None)[0])
    g = t["g"]
    print(f"block {name}: flippable share of E {100 * fr.share_e:.2f} %, of A' {100 * t['share_a']:.2f} %; gate {g.min():.2f} .. {g.max():.2f}, "
          f"mean |gate difference| of images 0 and 1 {(g[0] - g[1]).abs().mean():.3f}")
    assert fr.share_e <= FLIP_CAP, f"{name}: {100 * fr.share_e:.2f} % of the E elements are flippable"
    assert t["share_a"] <= FLIP_CAP, f"{name}: {100 * t['share_a']:.2f} % of the A' elements are flippable"
    assert g.min() > 0.01 and g.max() < 0.99 and g.max() - g.min() > 0.4, "the gates are saturated or all alike"
    assert (g[0] - g[1]).abs().mean() > 0.01, "the gates of two images do not differ"
    for mut, applies in MUTANTS.items():
        if not applies(c):
            continue
        Dm, Ym = mutant_outputs(c, d, fr, mut)
        tm = tail(c, d, fr, Dm)
        ratio = max(((Dm - fr.d64).abs() / fr.tolD).max().item(), ((Ym - tm["y"]).abs() / tm["tol"]).max().item())
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


def test_the_exact_kernel_passes_its_own_reference():
    """the reference's own rounding of D and Y (mutant None) lies inside the tolerance: 0.5 ulp is at most 2^-8 |ref|"""
    for name in ("edge_7x7_k5s1_silu_c256_m8_o48_rd128_res24", "inst07b_14x14_k3s1_lin_c128_m264_o128_rd18_res64"):
        c = CASES[name]
        d, fr = ref_of(name)
        D, Y = mutant_outputs(c, d, fr, None)
        t = tail(c, d, fr, D)
        assert ((D - fr.d64).abs() / fr.tolD).max() <= 1.0 and ((Y - t["y"]).abs() / t["tol"]).max() <= 1.0, name


def golden_block_layers():
    """[(model, (H, W, Cin, mid, Cout, k, stride, rd))]: every whole-block step the committed launch-plan golden records for the
    three convolutional backbones at 224 x 224, batch 256, default options; channel counts padded to 8 as the packer does."""
    from launch_plan_cases import decode_steps
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")))
    L, out = g["lists"], []
    for model in ("efficientnet_b3a", "rexnet_150", "rexnet_200"):
        first_op, n_ops, how = decode_steps(L[g["plans"][f"{model}|256|256|224x224|defaults|features"][0]])
        labels = L[g["profile_ops"][f"{model}|256|224x224"][0]]
        for f, n, h in zip(first_op, n_ops, how):
            if g["how"][h] != "block":
                continue
            assert n == 4
            a = re.match(r"pw (\d+)->(\d+) @(\d+)x(\d+)$", labels[f])
            b = re.match(r"dw k(\d) s(\d) C(\d+)", labels[f + 1])
            s = re.match(r"se C(\d+) rd(\d+)$", labels[f + 2])
            p = re.match(r"pw (\d+)->(\d+) @(\d+)x(\d+) gate( res)?$", labels[f + 3])
            cin, mid, H, W = (int(v) for v in a.groups())
            out.append((model, (H, W, pad8(cin), pad8(mid), pad8(int(p.group(2))), int(b.group(1)), int(b.group(2)), int(s.group(2))),
                        bool(p.group(5)), f, n))
    return out


def test_model_cases_agree_with_the_launch_plan():
    """For every whole-block step of the launch-plan golden (batch 256): the live mi355_model_plan still plans it whole-block, a
    model case has exactly its shape, and the path mi355_mbconv_block_how reports for it carries the step's k, stride, map width
    and expand k-steps."""
    from imageretrievalresearch_amd._lib import lib
    L = lib()
    layers = golden_block_layers()
    assert sum(m == "efficientnet_b3a" for m, *_ in layers) == 17 and len(layers) == 33      # whole-block launches per forward ...
    assert len({(m, s) for m, s, *_ in layers}) == len(MODEL_LAYERS)          # ... of 23 distinct shapes
    by_shape = {(c.model, c.shape[:8]): c for c in CASES.values() if c.model}
    MAX = 1024
    fo, no, hw = (ctypes.c_int * MAX)(), (ctypes.c_int * MAX)(), (ctypes.c_int * MAX)()
    plans = {}
    for model, shape, res, f, n in layers:
        if model not in plans:
            h, arena = ctypes.c_void_p(), ctypes.c_size_t(0)
            assert L.mi355_model_create(model.encode(), 0, ctypes.byref(h)) == 0
            cnt = L.mi355_model_plan(h, 256, 256, 224, 224, 0, MAX, fo, no, hw, ctypes.byref(arena))
            L.mi355_model_destroy(h)
            assert 0 < cnt <= MAX
            plans[model] = {fo[i]: (no[i], hw[i]) for i in range(cnt)}
        assert plans[model][f] == (n, 4), (model, shape)                      # MI355_PLAN_BLOCK
        c = by_shape[model, shape]
        assert (c.res_n > 0) == res, (model, shape)
        got = path_fields(_how(c.shape))
        H, W, cin, mid, cout, k, s, rd = shape
        assert (got["ks"], got["s"], got["wi"], got["kst"]) == (k, s, W, (cin + 31) // 32), (model, shape, got)
        assert got["act_d"] == (ACT_SILU if model.startswith("eff") else ACT_NONE)


# ------------------------------------------------------------------------------------------------------------------- GPU
def _run(c: Case, d: Data, norot=0):
    """One call of mi355_mbconv_block_ex -> (path, D [B][Ho][Wo][mid], Y [B][Ho][Wo][Cout], guards)."""
    from imageretrievalresearch_amd._lib import MbconvBlockArgs, check, lib, stream_ptr
    bf = lambda t: t.to(torch.bfloat16).to(DEV).contiguous()          # noqa: E731
    we, be = d.we_packed(c)
    wp, bp = d.wp_packed(c)
    keep = [bf(d.x), bf(we), be.to(DEV), bf(d.wd), d.bd.to(DEV), bf(d.w1), d.b1.to(DEV), bf(d.w2), d.b2.to(DEV), bf(wp), bp.to(DEV)]
    nD, nY = c.B * c.Pout * c.mid, c.B * c.Pout * c.Cout
    D = torch.full((nD + GUARD,), float("nan"), device=DEV, dtype=torch.bfloat16)
    Y = torch.full((nY + GUARD,), float("nan"), device=DEV, dtype=torch.bfloat16)
    ptr = dict(zip(("X", "We", "be", "Wd", "bd", "W1", "b1", "W2", "b2", "Wp", "bp"), (t.data_ptr() for t in keep)))
    a = MbconvBlockArgs(D=D.data_ptr(), Y=Y.data_ptr(), B=c.B, H=c.H, W=c.W, Cin=c.Cin, mid=c.mid, Cout=c.Cout, k=c.k, stride=c.stride,
                        rd=c.rd, act_e=ACT_SILU, act_d=c.act_d, se_act=c.se_act, a_relu6=c.a_relu6, has_res=int(c.res_n > 0),
                        res_n=c.res_n, norot=norot, **ptr)
    path = ctypes.c_int(-1)
    check(lib().mi355_mbconv_block_ex(ctypes.byref(a), ctypes.byref(path), stream_ptr(DEV)))
    torch.cuda.synchronize()
    Dh, Yh = D.cpu(), Y.cpu()
    return (path.value, Dh[:nD].view(c.B, c.Ho, c.Wo, c.mid), Yh[:nY].view(c.B, c.Ho, c.Wo, c.Cout), {"D": Dh[nD:], "Y": Yh[nY:]})


def _worst(got, ref, tol):
    ratio = (got - ref).abs() / tol
    i = int(ratio.argmax())
    return ratio.view(-1)[i].item(), tuple(int(j) for j in torch.unravel_index(torch.tensor(i), ratio.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_block_matches_float64(name):
    c = CASES[name]
    d, fr = ref_of(name)
    path, D, Y, guards = _run(c, d)
    assert path == c.code, f"{name}: ran path {path:#x} = {path_fields(path)}, expected {c.code:#x} = {c.f}"
    for k, g in guards.items():
        assert torch.isnan(g).all(), f"{name}: wrote past the end of {k}"
    for k, t in (("D", D), ("Y", Y)):
        bad = torch.isnan(t.float()).nonzero()
        assert bad.numel() == 0, f"{name}: {k} unwritten (or NaN) at (image, y, x, channel) {bad[0].tolist()}"
    wD, at = _worst(D.double(), fr.d64, fr.tolD)
    rel = (2.0 ** -8 * fr.d64[at].abs() / fr.tolD[at]).item()
    assert wD <= 1.0, (f"{name} {c.instance}: D |err| / tol {wD:.3f} at (image, y, x, channel) {at}: got {D[at].item()}, reference "
                       f"{fr.d64[at].item():.6f}; {100 * rel:.0f} % of the tolerance there is 2^-8 |d64| (the bf16 rounding of D), the "
                       f"rest the fp32 tap sum and the slack of the flippable E elements")
    t = tail(c, d, fr, D.double())
    wY, at = _worst(Y.double(), t["y"], t["tol"])
    terms = t["terms"][(slice(None),) + at]
    print(f"block {name:64s} {family(c):12s} {str(c.instance):24s} flippable E {100 * fr.share_e:.2f} % A' {100 * t['share_a']:.2f} %: "
          f"worst |err| / tol D {wD:.3f} Y {wY:.3f}")
    assert wY <= 1.0, (f"{name} {c.instance}: Y |err| / tol {wY:.3f} at (image, y, x, channel) {at}: got {Y[at].item()}, reference "
                       f"{t['y'][at].item():.6f}; the tolerance's largest part there is {TERMS[int(terms.argmax())]} "
                       f"({', '.join(f'{v:.2e}' for v in terms.tolist())})")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(rotation_cases()))
def test_bits_do_not_depend_on_the_batch_position(name):
    """ROT_B copies of one image: more than the periods of the slab, FC1-group and column-group rotations.  D and Y of every
    position equal those of position 0, and the whole output equals the one computed without any rotation (norot 15)."""
    c = rotation_cases()[name]
    d = Data(c)
    path, D, Y, guards = _run(c, d)
    assert path == c.code
    assert not torch.isnan(D.float()).any() and not torch.isnan(Y.float()).any()
    assert torch.isnan(guards["D"]).all() and torch.isnan(guards["Y"]).all()
    Di, Yi = D.view(torch.int16), Y.view(torch.int16)
    for b in range(1, c.B):
        assert torch.equal(Di[b], Di[0]), f"{name}: D of position {b} differs from position 0"
        assert torch.equal(Yi[b], Yi[0]), f"{name}: Y of position {b} differs from position 0"
    path2, D2, Y2, _ = _run(c, d, norot=15)
    assert path2 == path
    assert torch.equal(D2.view(torch.int16), Di) and torch.equal(Y2.view(torch.int16), Yi), f"{name}: norot 15 changes the bits"
