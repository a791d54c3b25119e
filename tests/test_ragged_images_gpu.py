"""Ragged batches of decoded uint8 images: ``preprocess.resize_batch`` and ``MI355Model.forward_images``
against the per-image tools they replace (``square_pad_normalize``, ``resize``, ``forward_uint8``) and the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import preprocess as opre

DEV = "cuda:0"
PAD_SHAPES = [(224, 224), (224, 150), (97, 224), (224, 223), (1, 224)]    # one longer side, odd remainders
# the source shapes of tests/test_preprocess.py::RESIZE_CASES, one ragged batch
RESIZE_SHAPES = [(300, 400), (224, 224), (100, 80), (640, 480), (225, 223), (1000, 37), (224, 500), (31, 224), (7, 5),
                 (513, 1027), (224, 224)]
MIX = [(375, 500), (480, 640), (512, 512), (1000, 37), (224, 224)]


def _img(seed, h, w):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8)


def _batch(shapes, seed=0):
    np_imgs = [_img(seed + 17 * i + 1, h, w) for i, (h, w) in enumerate(shapes)]
    return np_imgs, [torch.from_numpy(a).to(DEV) for a in np_imgs]


def _model(name, **kw):
    import imageretrievalresearch_amd as M
    return M.create_model(name, num_classes=0, **kw).to(DEV).eval()


# ---------------------------------------------------------------- "pad": SquarePad fused into the stem / patch embedding
@pytest.mark.gpu
@pytest.mark.parametrize("name,conv_input,tap", [("efficientnet_b3a", False, "stem"), ("efficientnet_b3a", True, "stem"),
                                                 ("rexnet_150", False, "stem"), ("swin_base_patch4_window7_224", False,
                                                                                 "patch_embed")])
def test_pad_is_bit_identical_to_square_pad_normalize(name, conv_input, tap):
    import imageretrievalresearch_amd as M
    from imageretrievalresearch_amd import preprocess as P
    _, imgs = _batch(PAD_SHAPES, seed=3)
    model = _model(name)
    wrapped = M.models.with_conv_input(model).to(DEV).eval() if conv_input else None
    x = P.square_pad_normalize(imgs)
    model.enable_taps(True)
    want = wrapped(x) if conv_input else model(x)
    want_tap = model.read_tap(tap)
    got = model.forward_images(imgs, "pad", conv_input=wrapped[0] if conv_input else None)
    got_tap = model.read_tap(tap)
    model.enable_taps(False)
    assert torch.equal(got_tap, want_tap)
    assert torch.equal(got, want)
    if not conv_input:
        assert torch.equal(model.forward_images(imgs, "pad", features=True), model.forward_features(x))
        # the packed form is the same batch
        assert torch.equal(model.forward_images(P.pack_images(imgs), "pad"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["efficientnet_b3a", "swin_base_patch4_window7_224"])
def test_pad_on_a_uniform_batch_equals_forward_uint8(name):
    _, imgs = _batch([(224, 180)] * 4, seed=5)
    model = _model(name)
    assert torch.equal(model.forward_images(imgs, "pad"), model.forward_uint8(torch.stack(imgs)))


@pytest.mark.gpu
def test_pad_refusals():
    import imageretrievalresearch_amd as M
    _, imgs = _batch([(224, 224), (200, 150)])
    eff = _model("efficientnet_b3a")
    swin = _model("swin_base_patch4_window7_224")
    with pytest.raises(M.MI355Error):
        eff.forward_images(imgs, "pad")                               # mixed longer sides
    with pytest.raises(M.MI355Error):
        swin.forward_images(imgs[1:], "pad")                          # S != 224
    with pytest.raises(M.MI355Error):
        swin.forward_images(imgs, "pad")
    with pytest.raises(M.MI355Error):
        swin.forward_images(imgs[:1], "pad", conv_input=M.models.ConvInput().to(DEV))
    with pytest.raises(M.MI355Error):
        eff.forward_images([imgs[0].cpu()], "pad")                    # host tensor
    with pytest.raises(M.MI355Error):
        eff.forward_images([imgs[0].float()], "pad")                  # not uint8
    with pytest.raises(M.MI355Error):
        eff.forward_images([imgs[0][:, :, :2].contiguous()], "pad")   # not HWC3
    with pytest.raises(M.MI355Error):
        eff.forward_images(imgs[:1], "crop")


# ---------------------------------------------------------------- resize_batch
@pytest.mark.gpu
@pytest.mark.parametrize("size", [(224, 224), (112, 300), (57, 75), (3, 2)])     # the last two: rows of 3 * w % 4 != 0 bytes
def test_resize_batch_is_bit_exact_with_pillow_and_the_per_image_resize(size):
    from imageretrievalresearch_amd import preprocess as P
    np_imgs, imgs = _batch(RESIZE_SHAPES, seed=11)
    got = P.resize_batch(imgs, size)
    assert got.shape == (len(imgs), size[0], size[1], 3) and got.dtype == torch.uint8
    assert torch.equal(got, torch.stack([P.resize(im, size) for im in imgs]))
    g = got.cpu().numpy()
    for b, a in enumerate(np_imgs):
        np.testing.assert_array_equal(g[b], opre.pil_resize_bilinear(a, *size), err_msg=str(a.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [255, 0, 37])
def test_resize_batch_pad_is_square_pad_then_pillow(fill):
    from imageretrievalresearch_amd import preprocess as P
    np_imgs, imgs = _batch(RESIZE_SHAPES, seed=13)
    g = P.resize_batch(P.pack_images(imgs), (224, 224), pad=True, fill=fill).cpu().numpy()
    for b, a in enumerate(np_imgs):
        np.testing.assert_array_equal(g[b], opre.pil_resize_bilinear(opre.square_pad(a, fill), 224, 224), err_msg=str(a.shape))


# ---------------------------------------------------------------- "resize" / "pad_resize" forwards
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["efficientnet_b3a", "swin_base_patch4_window7_224"])
def test_resize_forwards_equal_forward_uint8_on_the_per_image_result(name):
    from imageretrievalresearch_amd import preprocess as P
    np_imgs, imgs = _batch(MIX + [(300, 299)], seed=17)
    model = _model(name)
    stacked = torch.stack([P.resize(im, (224, 224)) for im in imgs])
    assert torch.equal(model.forward_images(imgs, "resize"), model.forward_uint8(stacked, mean=(0, 0, 0), std=(1, 1, 1)))
    padded = torch.stack([P.resize(torch.from_numpy(opre.square_pad(a)).to(DEV), (224, 224)) for a in np_imgs])
    assert torch.equal(model.forward_images(imgs, "pad_resize"), model.forward_uint8(padded))
    mean, std = (0.5, 0.4, 0.3), (0.2, 0.3, 0.4)
    assert torch.equal(model.forward_images(imgs, "resize", mean=mean, std=std), model.forward_uint8(stacked, mean=mean, std=std))


@pytest.mark.gpu
def test_resize_forward_conv_input_features_and_head():
    import imageretrievalresearch_amd as M
    from imageretrievalresearch_amd import preprocess as P
    _, imgs = _batch(MIX, seed=19)
    model = _model("efficientnet_b3a")
    conv = M.models.ConvInput().to(DEV)
    stacked = P.resize_batch(imgs, (256, 256), pad=True)
    assert torch.equal(model.forward_images(imgs, "pad_resize", size=256, conv_input=conv, features=True),
                       model.forward_uint8(stacked, conv_input=conv, features=True))

    class Head(torch.nn.Module):
        def forward(self, f):
            return torch.nn.functional.normalize(f, dim=1)[:, :5] * 2.0

    model.classifier = Head()
    got = model.forward_images(imgs, "pad_resize", size=256)
    assert got.shape == (len(imgs), 5) and torch.equal(got, model.forward_uint8(stacked))


# ---------------------------------------------------------------- invariance and stream ordering
def _b256(seed):
    shapes = [(224, 100 + (i * 37) % 125) if i % 2 else (100 + (i * 53) % 125, 224) for i in range(256)]
    return _batch(shapes, seed=seed)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("transform", ["pad", "resize"])
def test_shuffle_lanes_and_microbatch_keep_the_bits(transform):
    imgs = _b256(23) if transform == "pad" else _batch([MIX[i % len(MIX)] for i in range(256)], seed=29)[1]
    model = _model("efficientnet_b3a")
    want = model.forward_images(imgs, transform)
    perm = torch.randperm(len(imgs), generator=torch.Generator().manual_seed(1))
    assert torch.equal(model.forward_images([imgs[i] for i in perm.tolist()], transform), want[perm.to(DEV)])
    model.set_option("lanes", 2)
    got_lanes = model.forward_images(imgs, transform)
    model.set_option("lanes", 1)
    model.set_option("microbatch", 64)
    got_mb = model.forward_images(imgs, transform)
    model.set_option("microbatch", 0)
    assert torch.equal(got_lanes, want)
    assert torch.equal(got_mb, want)


@pytest.mark.gpu
@pytest.mark.parametrize("transform", ["pad", "resize", "pad_resize"])
def test_back_to_back_calls_without_a_synchronise(transform):
    model = _model("efficientnet_b3a")
    a = _batch(PAD_SHAPES * 3, seed=31)[1]
    b = _batch([(224, 61), (224, 224), (13, 224)] * 20, seed=37)[1]
    if transform != "pad":
        a = _batch(MIX * 3, seed=41)[1]
        b = _batch([(333, 77), (64, 2000), (999, 998), (5, 5)] * 10, seed=43)[1]
    want_a = model.forward_images(a, transform)
    torch.cuda.synchronize()
    want_b = model.forward_images(b, transform)
    torch.cuda.synchronize()
    got_a = model.forward_images(a, transform)
    got_b = model.forward_images(b, transform)
    got_a2 = model.forward_images(a, transform)
    torch.cuda.synchronize()
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b) and torch.equal(got_a2, want_a)
