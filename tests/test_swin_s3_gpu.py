"""swin_s3_base_224 on the GPU: the 14x14 window-attention kernel (k_win_attn14) against float64, and the whole model against
the bf16-simulated restatement of timm's forward (tests/swin_s3_ref.py).  Parity with timm itself is UNPINNED."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import swin_s3_ref as ref
from test_effnet_gpu import images, rel
from test_swin_s3_args import CASES, HD, make_data, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_TAP_SIM = 2e-2
TOL_EMB_FP32 = 4e-2
TOL_BLOCK_ISOLATED = {0: 2e-3, 1: 6e-3}     # as for swin_base (tests/test_swin_gpu.py)


def _attn(qkv, table, B, res, heads, window, shift=0):
    from imageretrievalresearch_amd._lib import check, lib, stream_ptr
    C = HD * heads
    dq, dt = qkv.to(DEV), table.to(DEV).contiguous()
    out = torch.full((B, res * res, C), float("nan"), device=DEV, dtype=torch.bfloat16)
    check(lib().mi355_window_attention_ws(dq.data_ptr(), dt.data_ptr(), out.data_ptr(), B, res, C, heads, window, shift,
                                          stream_ptr(DEV)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_window14_attention_matches_float64(name):
    B, res, heads, _ = CASES[name]
    qkv, table = make_data(name)
    got = _attn(qkv, table, B, res, heads, 14).cpu().double()
    assert torch.isfinite(got).all(), f"{name}: non-finite or unwritten outputs"
    want, tol = reference(name, qkv, table)
    ratio = (got - want).abs() / tol
    worst = ratio.max().item()
    print(f"win_attn14 {name:28s}: worst |err| / tol = {worst:.3f}")
    assert worst <= 1.0, f"{name}: worst |err| / tol {worst:.3f} at {np.unravel_index(ratio.argmax().item(), ratio.shape)}"


@pytest.mark.parametrize("res,heads,shift", [(28, 6, 3), (14, 12, 0), (7, 24, 0)])
def test_window7_through_the_new_entry_has_the_old_bits(res, heads, shift):
    from imageretrievalresearch_amd._lib import check, lib, stream_ptr
    g = torch.Generator().manual_seed(res * heads)
    C = HD * heads
    qkv = torch.randn(2, res * res, 3 * C, generator=g).bfloat16()
    table = torch.randn(169, heads, generator=g)
    a = _attn(qkv, table, 2, res, heads, 7, shift)
    b = torch.full_like(a, float("nan"))
    dq, dt = qkv.to(DEV), table.to(DEV).contiguous()
    check(lib().mi355_window_attention(dq.data_ptr(), dt.data_ptr(), b.data_ptr(), 2, res, C, heads, shift, stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.fixture(scope="module")
def setup():
    sd = ref.init_state_dict(6)
    model = M.create_model(ref.NAME).to(DEV).eval()
    model.load_state_dict(sd, strict=True)
    return sd, model


@pytest.mark.parametrize("fuse_ln", [1, 0])
def test_taps_match_bf16_sim(setup, fuse_ln):
    sd, model = setup
    x = torch.from_numpy(images(61, 2))
    taps = {}
    want = ref.forward_features(sd, x, sim_bf16=True, taps=taps)
    model.set_option("fuse_ln", fuse_ln)
    model.enable_taps(True)
    try:
        got = model.forward_features(x.to(DEV))
        for name, r in taps.items():
            t = model.read_tap(name).cpu().flatten(2).transpose(1, 2)
            assert t.shape == r.shape, (name, t.shape, r.shape)
            e = rel(t, r)
            assert e < TOL_TAP_SIM, f"tap {name}: rel L2 {e:.3e}"
    finally:
        model.enable_taps(False)
        model.set_option("fuse_ln", 1)
    assert got.shape == (2, 768)
    assert rel(got.cpu(), want) < TOL_TAP_SIM


def test_embedding_logits_and_head_identity(setup):
    sd, model = setup
    x = torch.from_numpy(images(63, 2))
    f32 = ref.forward_features(sd, x)
    emb = model.forward_features(x.to(DEV))
    assert rel(emb.cpu(), f32) < TOL_EMB_FP32
    assert torch.nn.functional.cosine_similarity(emb.cpu(), f32).min() > 0.999
    out = model(x.to(DEV))
    assert out.shape == (2, 1000)
    assert rel(out.cpu(), ref.forward(sd, x, sim_bf16=True)) < 3e-2
    assert torch.equal(out, model(x.to(DEV)))
    head = model.head
    model.head = torch.nn.Identity()
    try:
        e2 = model(x.to(DEV))
        assert e2.shape == (2, 768) and torch.equal(e2, emb)
    finally:
        model.head = head
    with pytest.raises(M.MI355Error):
        model(torch.zeros(1, 3, 192, 192, device=DEV))


@pytest.mark.parametrize("B,fuse_ln", [(2, 1), (2, 0), (128, 1), (128, 0)])
def test_each_block_on_the_references_own_input(setup, B, fuse_ln):
    sd, model = setup
    x = torch.from_numpy(images(67, 2))
    taps = {}
    ref.forward_features(sd, x, sim_bf16=True, taps=taps)
    order = list(taps.keys())
    assert order[0] == "patch_embed" and len(order) == 1 + 36 + 3
    model.set_option("fuse_ln", fuse_ln)
    model.enable_taps(True)
    try:
        for prev, cur in zip(order[:-1], order[1:]):
            t = taps[prev]
            L, C = t.shape[1], t.shape[2]
            side = int(round(L ** 0.5))
            src = t.transpose(1, 2).reshape(2, C, side, side).contiguous().to(DEV)
            if B > 2:
                src = src.repeat(B // 2, 1, 1, 1).contiguous()
            model.run_between_taps(prev, cur, src)
            got = model.read_tap(cur)
            if B > 2:
                g = got.view(B // 2, 2, *got.shape[1:])
                assert all(torch.equal(g[0], g[i]) for i in range(1, B // 2)), f"{cur}: result depends on the batch position"
                got = g[0]
            got = got.flatten(2).transpose(1, 2).cpu()
            e = rel(got, taps[cur])
            assert e < TOL_BLOCK_ISOLATED[fuse_ln], f"{prev} -> {cur} at B={B}, fuse_ln={fuse_ln}: rel L2 {e:.3e}"
    finally:
        model.enable_taps(False)
        model.set_option("fuse_ln", 1)


def test_chunking_does_not_change_the_bits():
    from imageretrievalresearch_amd import synth
    model = M.create_model(ref.NAME, num_classes=0, seed=6).to(DEV).eval()
    B = 128
    x = M.synth_fill(B * 3 * 224 * 224, 89, synth.UNIFORM, DEV).view(B, 3, 224, 224)
    want = model(x).clone()
    assert torch.isfinite(want).all()
    try:
        model.set_option("microbatch", 48)
        assert torch.equal(model(x), want)
        model.set_option("microbatch", 0)
        model.set_option("lanes", 2)
        assert torch.equal(model(x), want)
    finally:
        model.set_option("microbatch", 0)
        model.set_option("lanes", 1)


def test_forward_images_pad_matches_square_pad_normalize():
    """uint8 images through the 96-wide patch embedding's ragged and uniform forms: the same bits as the fp32 form on the
    SquarePad + Normalize batch (as tests/test_ragged_images_gpu.py does for swin_base)."""
    from imageretrievalresearch_amd import preprocess as P
    model = M.create_model(ref.NAME, num_classes=0, seed=3).to(DEV).eval()
    rng = np.random.RandomState(5)
    imgs = [torch.from_numpy(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV) for h, w in [(224, 150), (97, 224), (224, 224)]]
    x = P.square_pad_normalize(imgs)
    model.enable_taps(True)
    try:
        want = model(x)
        want_tap = model.read_tap("patch_embed").clone()
        got = model.forward_images(imgs, "pad")
        assert torch.equal(model.read_tap("patch_embed"), want_tap)
    finally:
        model.enable_taps(False)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    same = [imgs[0]] * 3
    assert torch.equal(model.forward_images(same, "pad"), model.forward_uint8(torch.stack(same)))
