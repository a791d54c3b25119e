"""swin_s3_base_224 without a GPU: registration, state-dict layout against tests/swin_s3_ref.py, parameter count, MACs, the
argument checks of mi355_window_attention_ws, and the float64 reference of the 14x14 window attention (used by
tests/test_swin_s3_gpu.py) checked against deliberate bugs."""
import math

import pytest
import torch

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd._lib import lib
from oracle import swin
from oracle.common import count_params
import swin_s3_ref as ref

WS, NTOK, HD = 14, 196, 32
TOL = 2.0 ** -8
MARGIN = 10.0

# name -> (B, res, heads, kind)
CASES = {
    "res14_b1_normal": (1, 14, 12, "normal"),
    "res28_b1_normal": (1, 28, 12, "normal"),
    "res14_b3_normal": (3, 14, 12, "normal"),
    "res28_b3_normal": (3, 28, 12, "normal"),
    "res14_b1_peaked": (1, 14, 12, "peaked"),
    "res28_b1_identical_keys": (1, 28, 12, "identical_keys"),
    "res14_b3_large_table": (3, 14, 12, "large_table"),
}


def _windows(t, B, res, heads):
    return swin.window_partition(t.view(B, res, res, -1), WS).view(-1, NTOK, heads, HD).transpose(1, 2)


def make_data(name):
    """(qkv bf16 [B][res*res][3C], bias table fp32 [729][heads]), seeded per case."""
    B, res, heads, kind = CASES[name]
    C = HD * heads
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    qkv = torch.randn(B, res * res, 3 * C, generator=g)
    table = torch.randn((2 * WS - 1) ** 2, heads, generator=g) * 0.5
    if kind == "peaked":                          # largest logit about 30: softmax close to one-hot
        q, k = qkv[..., :C].bfloat16().double(), qkv[..., C:2 * C].bfloat16().double()
        mx = float((_windows(q, B, res, heads) @ _windows(k, B, res, heads).transpose(-1, -2)).abs().max()) * HD ** -0.5
        qkv[..., :2 * C] *= math.sqrt(30.0 / mx)
    elif kind == "identical_keys":
        qkv[..., C:2 * C] = qkv[0, 0, C:2 * C]
        table = table * 4.0
    elif kind == "large_table":
        table = torch.randn((2 * WS - 1) ** 2, heads, generator=g) * 8.0
    return qkv.bfloat16(), table.float()


MUTANTS = ["bias_left_out", "bias_dy_dx_swapped", "bias_7x7_formula", "last_key_tile_dropped", "padded_keys_in_softmax"]


def _index_7x7_formula():
    """the 7x7 kernel's index (dy + ws-1) * (2ws-1) + (dx + ws-1) evaluated with ws = 7 on 14x14 coordinates, wrapped into the
    729-row table: what a kernel that kept the 7x7 formula would read."""
    c = torch.stack(torch.meshgrid([torch.arange(WS), torch.arange(WS)], indexing="ij")).flatten(1)
    rel = c[:, :, None] - c[:, None, :]
    return ((rel[0] + 6) * 13 + (rel[1] + 6)) % ((2 * WS - 1) ** 2)


def reference(name, qkv, table, mutant=None):
    """(out, tol) [B][res*res][C] float64; `mutant` names a deliberate bug."""
    B, res, heads, _ = CASES[name]
    C = HD * heads
    x = qkv.double().view(B, res, res, 3 * C)
    win = swin.window_partition(x, WS).view(-1, NTOK, 3, heads, HD).permute(2, 0, 3, 1, 4)   # [3][Bw][heads][196][32]
    q, k, v = win[0], win[1], win[2]
    attn = (q * HD ** -0.5) @ k.transpose(-2, -1)
    if mutant != "bias_left_out":
        idx = swin.relative_position_index(WS)
        if mutant == "bias_dy_dx_swapped":
            idx = (idx % 27) * 27 + idx // 27
        elif mutant == "bias_7x7_formula":
            idx = _index_7x7_formula()
        bias = table.double()[idx.reshape(-1)].view(NTOK, NTOK, heads).permute(2, 0, 1)
        attn = attn + bias.unsqueeze(0)
    if mutant == "padded_keys_in_softmax":        # the 12 padded keys (196..207) not masked: zero values, each at the row's top logit
        attn = torch.cat([attn, attn.amax(-1, keepdim=True).expand(*attn.shape[:-1], 12)], -1)
        v = torch.cat([v, torch.zeros(*v.shape[:-2], 12, HD, dtype=v.dtype)], -2)
    p = torch.softmax(attn, dim=-1)
    if mutant == "last_key_tile_dropped":
        p = p.clone()
        p[..., 192:NTOK] = 0.0
    vmax = v.abs().amax(dim=-2, keepdim=True).expand(-1, -1, NTOK, -1)

    def unwindow(t):
        return swin.window_reverse(t.transpose(1, 2).reshape(-1, WS, WS, C), WS, res, res).reshape(B, res * res, C)
    out = unwindow(p @ v)
    return out, TOL * unwindow(vmax) + TOL * out.abs()


@pytest.mark.parametrize("name", list(CASES))
def test_mutants_are_far_outside_the_tolerance(name):
    qkv, table = make_data(name)
    out, tol = reference(name, qkv, table)
    for mut in MUTANTS:
        m, _ = reference(name, qkv, table, mut)
        ratio = ((m - out).abs() / tol).max().item()
        assert ratio > MARGIN, f"{name}: mutant {mut} only {ratio:.1f}x the tolerance"


def test_registered():
    assert "swin_s3_base_224" in M.list_models()
    assert "swin_base_patch4_window7_224" in M.list_models()


def test_parameter_counts():
    assert sum(p.numel() for p in M.create_model(ref.NAME).parameters()) == 71125762
    assert sum(p.numel() for p in M.create_model(ref.NAME, num_classes=0).parameters()) == 70356762
    assert count_params(ref.init_state_dict(1)) == 71125762


def test_state_dict_keys_shapes_and_order_match_timm():
    m = M.create_model(ref.NAME)
    want = ref.init_state_dict(4)
    got = m.state_dict()
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert tuple(got[k].shape) == tuple(want[k].shape), k
    m.load_state_dict(want, strict=True)
    for k in want:
        if k.endswith("relative_position_index") or k.endswith("attn_mask"):
            assert torch.equal(m.state_dict()[k].float(), want[k].float()), k


def test_index_and_mask_buffers():
    sd = M.create_model(ref.NAME, num_classes=0).state_dict()
    sides = {s: tuple(sd[f"layers.{s}.blocks.0.attn.relative_position_index"].shape) for s in range(4)}
    assert sides == {0: (49, 49), 1: (49, 49), 2: (196, 196), 3: (49, 49)}
    masks = sorted(k for k in sd if k.endswith("attn_mask"))
    assert masks == sorted(f"layers.{s}.blocks.1.attn_mask" for s in (0, 1))
    assert tuple(sd["layers.0.blocks.1.attn_mask"].shape) == (64, 49, 49)
    assert tuple(sd["layers.1.blocks.1.attn_mask"].shape) == (16, 49, 49)
    assert tuple(sd["layers.2.blocks.0.attn.relative_position_bias_table"].shape) == (729, 12)
    assert torch.equal(sd["layers.2.blocks.0.attn.relative_position_index"], swin.relative_position_index(14))


def test_swin_base_table_is_unchanged():
    sd = swin.init_state_dict(2)
    m = M.create_model("swin_base_patch4_window7_224")
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    assert sum(p.numel() for p in m.parameters()) == 87768224


def test_macs():
    assert abs(M.create_model(ref.NAME, num_classes=0).traffic(1)["macs"] / 1e9 - 13.654) < 1e-3


def test_window_attention_ws_argument_errors():
    L = lib()
    p = 4096                                           # a non-null, aligned fake pointer: every call below is refused first
    cases = [
        ((None, p, p, 1, 14, 384, 12, 14, 0), b"null"),
        ((p, None, p, 1, 14, 384, 12, 14, 0), b"null"),
        ((p, p, None, 1, 14, 384, 12, 14, 0), b"null"),
        ((p, p, p, 1, 14, 384, 12, 8, 0), b"window"),
        ((p, p, p, 1, 14, 384, 12, 0, 0), b"window"),
        ((p, p, p, 0, 14, 384, 12, 14, 0), b"bad shape"),
        ((p, p, p, 1, 21, 384, 12, 14, 0), b"bad shape"),
        ((p, p, p, 1, 7, 384, 12, 14, 0), b"bad shape"),
        ((p, p, p, 1, 14, 380, 12, 14, 0), b"32 * heads"),
        ((p, p, p, 1, 14, 0, 0, 14, 0), b"32 * heads"),
        ((p, p, p, 1, 14, 384, 12, 14, 3), b"shift"),
        ((p + 8, p, p, 1, 14, 384, 12, 14, 0), b"aligned"),
        ((p, p, p + 8, 1, 14, 384, 12, 14, 0), b"aligned"),
        ((p, p, p, 1, 28, 384, 12, 7, 5), b"shift"),    # window 7: mi355_window_attention's own checks and messages
        ((p, p, p, 1, 30, 384, 12, 7, 0), b"multiple of 7"),
    ]
    for args, msg in cases:
        assert L.mi355_window_attention_ws(*args, None) != 0, args
        err = L.mi355_last_error()
        assert msg in err, (args, err)
