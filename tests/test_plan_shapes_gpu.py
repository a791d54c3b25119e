"""Every block of efficientnet_b3a and rexnet_100 / 130 / 150 / 200 alone on the oracle's input, at the input sizes and batch
sizes of tests/plan_shapes_ref.py: odd and non-square maps (225 x 231, 300 x 300, 160 x 224, 288 x 224, 256 x 320), 32 x 32
images whose last stage has M = B rows, and a batch ladder on both sides of every dispatch edge of `launch_gemm_bf16`, of the
split-K choice and of `fuse_block_min_batch`.  What is compared is the executor's per-shape arithmetic (plan, arena slots, squeeze
counts, band rows, stride-2 outputs of odd maps), which the kernel tests do not run and the isolated-block tests run at 224 only.

Limits of the library that the table respects: H, W >= 32 (`forward`), nothing else - a case the library refuses with MI355Error
fails.  The weights are the seeded state dicts of the isolated-block tests, for the blocks run alone with both SE matrices
scaled by 4 (plan_shapes_ref.py says why); the bounds are the project's whole-tensor TOL_BLOCK_ISOLATED and the slice
tolerance max(that, 4 N0) of plan_shapes_ref.py, which comes from the oracle's own fp32 / float64 noise and from nothing
measured here."""
import functools

import pytest
import torch

import imageretrievalresearch_amd as M
import plan_shapes_ref as P
from test_effnet_gpu import images, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def gpu_model(name, sharpen=True):
    model = M.create_model(name).to(DEV).eval()
    model.load_state_dict(P.state_dict(name, sharpen), strict=True)
    return model


@functools.lru_cache(maxsize=None)
def gpu_taps(name, H, W):
    """the oracle's taps of the two images, computed once per (model, size) and moved to the GPU once"""
    return {k: v.to(DEV) for k, v in P.oracle_taps(name, H, W).items()}


@functools.lru_cache(maxsize=None)
def gpu_head_plain(name, H, W):
    """the oracle's feature map of the two images under the plain state dict, for the whole-network comparison"""
    return P.oracle_taps(name, H, W, sharpen=False)["head"].to(DEV)


def repeated(t, B):
    """the two images (or the first alone) repeated to a batch of B"""
    return t[:1].contiguous() if B == 1 else t.repeat((B + 1) // 2, 1, 1, 1)[:B].contiguous()


def repeats_agree(got, B):
    """0-d bool tensor: every repeat of the two images equals the first bit for bit"""
    if B <= 2:
        return torch.ones((), dtype=torch.bool, device=got.device)
    full = B // 2
    g = got[:2 * full].view(full, 2, *got.shape[1:])
    same = (g == g[:1]).all()
    return same & (got[-1] == got[0]).all() if B % 2 else same


@pytest.mark.parametrize("name,H,W,B", P.ALL_CASES)
def test_each_block_on_the_oracles_input(name, H, W, B):
    model, taps = gpu_model(name), gpu_taps(name, H, W)
    order = list(taps)
    assert order[0] == "stem" and order[-1] == "head"
    n = min(B, 2)
    rows = []
    model.enable_taps(True)
    try:
        for prev, cur in zip(order[:-1], order[1:]):
            src = repeated(taps[prev], B)
            model.run_between_taps(prev, cur, src)
            got = model.read_tap(cur)
            del src
            assert got.shape == (B,) + tuple(taps[cur].shape[1:]), (cur, got.shape)
            rows.append(torch.cat([P.slice_worst(got[:n], taps[cur][:n]), repeats_agree(got, B).double()[None]]))
            del got
    finally:
        model.enable_taps(False)
    res = torch.stack(rows).cpu()                  # [blocks][whole, rows, columns, channel groups, repeats agree]
    tol_whole, tol_slice = P.TOL_BLOCK_ISOLATED[P.family(name)], P.slice_tol(name)
    for cur, r in zip(order[1:], res.tolist()):
        print(f"  {cur:12s} whole {r[0] / tol_whole:.3f} rows {r[1] / tol_slice:.3f} columns {r[2] / tol_slice:.3f} "
              f"channel groups {r[3] / tol_slice:.3f} (of the tolerance)")
    wi, si = int(res[:, 0].argmax()), int(res[:, 1:4].max(1).values.argmax())
    print(f"PLAN_SHAPES {name} {H}x{W} B={B}: worst whole {res[wi, 0] / tol_whole:.3f} at {order[1 + wi]}, "
          f"worst slice {res[si, 1:4].max() / tol_slice:.3f} at {order[1 + si]}")
    for cur, r in zip(order[1:], res.tolist()):
        assert r[4] == 1.0, f"{name} {H}x{W} B={B} {cur}: the result depends on the batch position"
        assert r[0] < tol_whole, f"{name} {H}x{W} B={B} {cur}: rel L2 {r[0]:.3e}"
        assert max(r[1:4]) < tol_slice, f"{name} {H}x{W} B={B} {cur}: worst slice (rows, columns, channel groups) {r[1:4]}"


@pytest.mark.parametrize("name,H,W,B", [(m, H, W, B) for m, H, W in P.ALL_SIZES for B in P.POOLED_B])
def test_pooled_path(name, H, W, B):
    """model.embed against the pooled oracle, the fused head + GAP bit-identical to head conv -> GAP (HW = 1, 35, 49, 63, 64,
    80 and 100 here), every repeat of the two images the same bits, and forward_features' shape the oracle's.  Whole network, so
    the plain state dict of the tests at 224 (plan_shapes_ref.py: the sharpened gates are for blocks run alone)."""
    model, head = gpu_model(name, False), gpu_head_plain(name, H, W)
    x = repeated(torch.from_numpy(images(P.IMAGE_SEED[P.family(name)], 2, H, W)).to(DEV), B)
    want = P.pool(head)
    try:
        model.set_option("fuse_head_gap", 0)
        emb0, log0 = model.embed(x)
        model.set_option("fuse_head_gap", 1)
        emb1, log1 = model.embed(x)
    finally:
        model.set_option("fuse_head_gap", 1)
    assert emb1.shape == (B, want.shape[1])
    assert torch.equal(emb0, emb1) and torch.equal(log0, log1)
    assert bool(repeats_agree(emb1, B))
    e = rel(emb1[:2], want)
    print(f"PLAN_SHAPES_POOLED {name} {H}x{W} B={B}: embedding rel L2 {e:.3e} (HW = {head.shape[2] * head.shape[3]})")
    assert e < P.TOL_EMB_SIM
    fm = model.forward_features(x)
    assert fm.shape == (B,) + tuple(head.shape[1:])
