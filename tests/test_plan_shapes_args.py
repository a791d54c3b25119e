"""CPU checks of tests/plan_shapes_ref.py: the case table resolves to plans that reach every way a conv step can run away from
224 x 224, the slice metric does what it says, the recorded noise floor holds, and each modelled bug is far outside the slice
tolerance.  Host only: plans need neither packed weights nor a GPU."""
import pytest
import torch

import plan_shapes_ref as P
from imageretrievalresearch_amd import create_model

CONV_KINDS = {"op", "fused_late", "sweep", "band", "block", "head_gap"}
# These reach 10x the tolerance on EVERY block they apply to.  The other two ("squeeze_drops_last_row",
# "gate_from_neighbour_image") act through the SE gate alone: they reach it on some block of every (model, size) - best block
# 44x ... 204x - but not on every block (EfficientNet's 112 / 56-row blocks move by 0.3x: one row in 113 of a squeeze whose gate
# passes a tenth of a relative change on).  A block-level bound cannot do better; the squeeze itself is bounded elementwise in
# tests/test_mbconv_front_gpu.py, tests/test_conv_paths_gpu.py and tests/test_mbconv_block_gpu.py.
EVERY_BLOCK = {"stride2_phase_shifted", "last_row_from_the_row_above", "last_column_replicated", "squeeze_over_input_pixel_count",
               "last_8_channels_zero", "residual_on_every_column"}


def test_the_table_is_the_one_the_header_states():
    assert P.LADDERS[(225, 231)] == (1, 2, 21, 83, 84, 95, 96, 97, 256)
    assert P.LADDERS[(32, 32)] == (1, 64, 65, 1023, 1024, 1025)
    assert P.LADDERS[(224, 224)] == (1, 21, 83, 84, 95, 97)
    others = [s for s in P.LADDERS if s not in ((225, 231), (32, 32), (224, 224))]
    assert sorted(others) == [(160, 224), (256, 320), (288, 224), (300, 300)] and all(P.LADDERS[s] == (2, 96, 256) for s in others)
    assert len(P.cases("efficientnet_b3a")) == len(P.cases("rexnet_200")) == 33
    for m in P.TRIMMED:
        assert P.sizes(m) == [(225, 231), (224, 224), (160, 224)] and len(P.cases(m)) == 18
    assert len(P.ALL_CASES) == 120 and len(P.ALL_SIZES) == 23


def test_every_case_resolves_a_plan_and_every_kind_is_reached_off_224():
    seen, seen224 = {}, {}
    for model in P.MODELS:
        m = create_model(model, num_classes=0)
        n_ops = sum(n for _, n, _ in m.plan(1)[0])
        for H, W, B in P.cases(model):
            for pooled in (True, False):
                steps, arena = m.plan(B, H, W, pooled=pooled)
                assert arena > 0 and steps[0][0] == 0 and sum(n for _, n, _ in steps) == n_ops, (model, H, W, B)
                assert all(steps[i + 1][0] == steps[i][0] + steps[i][1] for i in range(len(steps) - 1)), (model, H, W, B)
                for _, _, how in steps:
                    (seen if (H, W) != (224, 224) else seen224).setdefault((model, how), (H, W, B))
        print(model, {how: at for (mm, how), at in sorted(seen.items()) if mm == model})
        # every model reaches these away from 224 x 224 on its own channels ...
        assert {how for mm, how in seen if mm == model} >= {"op", "fused_late", "block", "head_gap"}, model
    # ... the band kernel where a model has a layer it wins on (not rexnet_130 / 150 at their three sizes) ...
    assert {mm for mm, how in seen if how == "band"} >= {"efficientnet_b3a", "rexnet_200"}
    # ... and "sweep" nowhere: the row-sweep kernel's shape classes are the square 112 / 56 / 28 maps (sw_class,
    # csrc/sweep_mbconv.hip), which of the table's sizes only 224 x 224 gives; the ladder at 224 does run it.
    assert {how for _, how in seen} == CONV_KINDS - {"sweep"}
    assert {mm for mm, how in seen224 if how == "sweep"} == set(P.MODELS)


def test_slices_merge_up_to_4096_elements_and_a_dead_slice_cannot_blow_up():
    idx, ng = P._groups(5, 2 * 136 * 7)          # a 5 x 7 map of 136 channels, two images: three rows make 4096, two are left over
    assert ng == 1 and idx.tolist() == [0] * 5
    idx, ng = P._groups(113, 2 * 24 * 116)       # 5568 elements a row: nothing merged
    assert ng == 113 and idx.tolist() == list(range(113))
    idx, ng = P._groups(7, 2000)                 # three rows a slice, the seventh joins the second slice
    assert ng == 2 and idx.tolist() == [0, 0, 0, 1, 1, 1, 1]
    g = torch.Generator().manual_seed(1)
    R = torch.randn(2, 24, 40, 40, generator=g)
    assert float(P.slice_worst(R, R).max()) == 0.0
    G = R.clone()
    G[:, :, -1] = R[:, :, -2]                    # one wrong row: the whole tensor moves by sqrt(2 / 40), and the last row slice
    w = P.slice_worst(G, R)                      # (1920 elements a row: rows 36 .. 39 are one slice) by sqrt(2 / 4)
    assert 0.2 < float(w[0]) < 0.25 and 0.65 < float(w[1]) < 0.76 and float(w[2]) < 0.3 and float(w[3]) < 0.3
    R2 = R.clone()
    R2[:, 8:16] = 0                              # a dead channel group: its denominator is a quarter of the tensor's rms
    G2 = R2.clone()
    G2[:, 8:16] = 1e-3 * R[:, 8:16]
    w = P.slice_worst(G2, R2)
    rms = float(R2.double().pow(2).mean().sqrt())
    assert float(w[3]) == pytest.approx(1e-3 * float(R[:, 8:16].double().pow(2).mean().sqrt()) / (0.25 * rms), rel=1e-6)


def test_the_slice_tolerance_is_four_noise_floors_or_the_whole_tensor_bound():
    assert P.slice_tol("efficientnet_b3a") == max(1.5e-3, 4 * P.N0["effnet"])
    assert P.slice_tol("rexnet_130") == max(2e-3, 4 * P.N0["rexnet"])


@pytest.mark.parametrize("model,H,W", P.ALL_SIZES)
def test_noise_floor_holds_and_every_bug_is_ten_tolerances_out(model, H, W):
    """The oracle's fp32 / float64 flip noise on this (model, size) stays under the recorded N0 on every slice, and each modelled bug moves some slice by more than 10x the slice tolerance."""
    taps = P.oracle_taps(model, H, W)
    nf = torch.stack(list(P.noise_floor(model, H, W, taps).values())).max(0).values
    print(f"{model} {H}x{W}: noise whole {nf[0]:.3e} rows {nf[1]:.3e} columns {nf[2]:.3e} channel groups {nf[3]:.3e}")
    assert float(nf.max()) <= P.N0[P.family(model)]
    tol = P.slice_tol(model)
    for mut, moved in P.mutant_moves(model, H, W, taps).items():
        if not moved:
            # the only bugs without a target: the partial residual in EfficientNet
            assert mut == "residual_on_every_column" and P.family(model) == "effnet", (mut, model, H, W)
            continue
        lo, hi = min(moved, key=moved.get), max(moved, key=moved.get)
        print(f"  {mut}: {len(moved)} blocks, {moved[lo] / tol:.1f}x at {lo} ... {moved[hi] / tol:.1f}x at {hi}")
        assert moved[hi] > 10 * tol, (mut, hi, moved[hi] / tol)
        if mut in EVERY_BLOCK:
            assert moved[lo] > 10 * tol, (mut, lo, moved[lo] / tol)
