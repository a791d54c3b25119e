"""The two ends of the conv backbones against float64, kernel by kernel: k_stem and k_stem_u8 (csrc/conv_kernels.hip), k_head_gap
(csrc/gemm_bf16.hip), k_gap, k_pool_linear and the two layout kernels every tap and run_between_taps goes through.

Before this file the stem was only compared bit for bit with its uint8 twin (and the twin with the chain that ends in the stem),
the fused head + GAP only with head conv -> k_gap at the model's own shapes, and the pooling and layout kernels with nothing
directly.  Each case here is one call of a developer entry (mi355_stem_ex, mi355_head_gap_ex, mi355_gap, mi355_pool_linear,
mi355_nhwc_to_nchw, mi355_nchw_to_nhwc) at a shape that reaches a branch the models' shapes do not; the entries report the
instantiation that ran and the test asserts it.  The references (tests/stem_head_ref.py) are numpy float64 on the operands the
kernel reads.  Every image of a case has its own scale and offset, every output is followed by a NaN guard of 256 elements that
must stay untouched, and each test prints its worst |err| / tol.

Tolerances (TOL_REL = 2^-8: one bf16 rounding; `mag` = the sum of absolute products and bias, through the activations'
derivative bounds):
    stem              |out - ref| <= 2^-8 |ref| + 2^-18 mag
        28 fp32 terms (27 taps and the bias): below 28 * 2^-24 mag < 2^-19 mag; 2^-18 leaves a factor 2, as in the depthwise
        test.  With conv_input the conv_input stage's own 2^-18 mag, times SiLU's 1.1, is carried through |w_stem|.
    k_gap (check b)   |pooled - mean| <= (HW + 2) 2^-24 mean_i |x_i|  on the GPU's own bf16 input
        the worst case of HW sequential fp32 additions, the rounding of 1 / HW and the product; nothing is rounded to bf16.
    head + GAP (c)    |pooled - ref| <= mean_i(2^-8 |ref_i| + 2^-20 mag_i) + (HW + 2) 2^-24 mean_i |ref_i|
        against the float64 head that rounds nothing; (a) is the bit equality with mi355_gemm_bf16_ex -> mi355_gap that the
        kernel's header promises.
    k_pool_linear     pooled_out as (b); out within 2^-18 sum_c |w p| of the float64 Linear of the kernel's own pooled values
        rounded to bf16: the worst case (C / 64 + 7) 2^-24 at the largest C here.
    layout kernels    exact.  A NaN must come out as a NaN; its payload is not compared (torch's own CPU conversion gives
                      0x7fc0 on its scalar path and 0xffff on its vector path).
Measured worst |err| / tol on the MI355X: stem 0.99 (fp32 form), 0.98 / 0.97 (uint8 form without / with conv_input): the output's
own bf16 rounding reaches 1 just above a power of two; head + GAP (a) bits equal in every case, (b) 0.053, (c) 0.79 at HW = 1;
k_gap 0.19; k_pool_linear 0.23 (pooled_out) and 0.003 (out)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import stem_head_ref as R

DEV = "cuda:0"
GUARD = R.GUARD
pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _lib():
    from imageretrievalresearch_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bf16_dev(values):
    """fp32 array holding bf16 values -> bf16 tensor on the device (exact)."""
    return _dev(np.asarray(values, np.float32)).to(torch.bfloat16)


def _guarded(n, dtype):
    return torch.full((n + GUARD,), float("nan"), device=DEV, dtype=dtype)


def _split(buf, shape, what):
    """(values as a CPU tensor of `shape`, after asserting the guard untouched)."""
    t = buf.cpu()
    n = math.prod(shape)
    assert torch.isnan(t[n:].float()).all(), f"{what}: wrote past the end"
    return t[:n].view(shape)


def _bits(t_bf16):
    return t_bf16.contiguous().view(torch.int16).numpy().view(np.uint16)


def _f3(v):
    return (ctypes.c_float * 3)(*v)


def _stem_call(out_shape, want_path, what, **kw):
    """One mi355_stem_ex call -> out [B][Ho][Wo][Cout] bf16 (CPU), guard checked, path asserted."""
    L = _lib()
    out = _guarded(math.prod(out_shape), torch.bfloat16)
    a = L.StemExArgs(out=out.data_ptr(), **kw)
    path = ctypes.c_int(-1)
    L.check(L.lib().mi355_stem_ex(ctypes.byref(a), ctypes.byref(path), L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert path.value == want_path, f"{what}: ran path {path.value:#x}, expected {want_path:#x}"
    got = _split(out, out_shape, what)
    bad = torch.isnan(got.float()).nonzero()
    assert bad.numel() == 0, f"{what}: unwritten at (image, y, x, channel) {bad[0].tolist()}"
    return got


def _check(got, ref, tol, what, where):
    w, at = R.worst(got, ref, tol)
    assert w <= 1.0, f"{what}: |err| / tol {w:.3f} at {where} {at}"
    return w


# -------------------------------------------------------------------------------------------------------------- stem, fp32
@pytest.mark.parametrize("name", list(R.STEM_CASES))
def test_stem_f32_matches_float64(name):
    c = R.STEM_CASES[name]
    d = R.StemData(c)
    x, w, bias = _dev(d.x), _dev(d.w), _dev(d.bias)
    Ho, Wo = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    got = _stem_call((c.B, Ho, Wo, c.Cout), c.path, name, x=x.data_ptr(), B=c.B, H=c.H, W=c.W, w=w.data_ptr(), bias=bias.data_ptr(),
                     Cout=c.Cout, act=c.act)
    y, mag = R.stem(d.x, d.w, d.bias, c.act)
    worst = _check(got.float().numpy(), y, R.stem_tol(y, mag), name, "(image, y, x, channel)")
    print(f"stem f32 {name:28s} path {c.path} B={c.B} {c.H}x{c.W} Cout={c.Cout} act={c.act}: worst |err| / tol = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------- stem, uint8
class _U8Run:
    """The device operands of one uint8 case and the calls on them."""

    def __init__(self, c, d):
        self.c, self.d = c, d
        self.w, self.bias = _dev(d.w), _dev(d.bias)
        self.cw = _dev(d.cw) if c.conv_input else None
        self.mean, self.std = _f3(c.mean), _f3(c.std)
        self.Ho = (c.S - 1) // 2 + 1
        self.imgs = [_dev(im) for im in d.imgs]

    def common(self):
        c = self.c
        return dict(fill=c.fill, mean=self.mean, stdv=self.std, conv_input_w=self.cw.data_ptr() if c.conv_input else None,
                    w=self.w.data_ptr(), bias=self.bias.data_ptr(), Cout=c.Cout, act=c.act)

    def uniform(self, idx, what):
        """The uniform uint8 form on images idx (all of one size)."""
        c = self.c
        h, w = c.sizes[idx[0]]
        batch = torch.stack([self.imgs[i] for i in idx]).contiguous()
        path = R.STEM_PATHS["U8"] | (R.STEM_PATHS["CONV_INPUT"] if c.conv_input else 0)
        return _stem_call((len(idx), self.Ho, self.Ho, c.Cout), path, what, images=batch.data_ptr(), B=len(idx), H=h, W=w,
                          **self.common())

    def ragged(self, what):
        c = self.c
        gap = [0, 5, 3, 1]                                   # bytes between the images: no image start is aligned
        desc, chunks, off = [], [], 7
        for i, im in enumerate(self.d.imgs):
            chunks.append(np.zeros(off - sum(len(x) for x in chunks), np.uint8))
            chunks.append(im.reshape(-1))
            desc.append((off, im.shape[0], im.shape[1]))
            off += im.size + gap[i % 4]
        packed = _dev(np.concatenate(chunks))
        dh = np.ascontiguousarray(np.array(desc, np.int64))
        dd = _dev(dh)
        return _stem_call((len(desc), self.Ho, self.Ho, c.Cout), c.path, what, images=packed.data_ptr(), images_bytes=packed.numel(),
                          desc_host=dh.ctypes.data, desc_dev=dd.data_ptr(), B=len(desc), H=c.S, W=c.S, **self.common())

    def chain(self, what):
        """mi355_square_pad_normalize (-> mi355_conv_input_silu) -> the fp32 form."""
        L = _lib()
        c, S, B = self.c, self.c.S, len(self.imgs)
        P = torch.full((B, 3, S, S), float("nan"), device=DEV)
        for b, im in enumerate(self.imgs):
            L.check(L.lib().mi355_square_pad_normalize(im.data_ptr(), im.shape[0], im.shape[1], c.fill, self.mean, self.std,
                                                       P[b].data_ptr(), L.stream_ptr(DEV)))
        if c.conv_input:
            Q = torch.full_like(P, float("nan"))
            L.check(L.lib().mi355_conv_input_silu(P.data_ptr(), self.cw.data_ptr(), B, S, S, Q.data_ptr(), L.stream_ptr(DEV)))
            P = Q
        path = R.STEM_PATHS["F32_LOAD16" if S % 4 == 0 else "F32_LOAD4"]
        return _stem_call((B, self.Ho, self.Ho, c.Cout), path, what, x=P.data_ptr(), B=B, H=S, W=S, w=self.w.data_ptr(),
                          bias=self.bias.data_ptr(), Cout=c.Cout, act=c.act)


@pytest.mark.parametrize("name", list(R.U8_CASES))
def test_stem_u8_matches_float64_and_its_promised_bits(name):
    c = R.U8_CASES[name]
    d = R.U8Data(c, name)
    run = _U8Run(c, d)
    B = len(c.sizes)
    got = run.ragged(name) if c.ragged else run.uniform(list(range(B)), name)
    y, tol = d.reference(c)
    worst = _check(got.float().numpy(), y, tol, name, "(image, y, x, channel)")
    print(f"stem u8  {name:28s} path {c.path:#x} B={B} S={c.S} fill={c.fill} Cout={c.Cout}: worst |err| / tol = {worst:.3f}")
    # the kernel header's promise: the same fp32 operation order as the separate kernels, so the same bits
    chain = run.chain(name + " (chain)")
    assert torch.equal(_split_bits(got), _split_bits(chain)), f"{name}: uint8 form differs from square_pad_normalize -> " \
        f"{'conv_input_silu -> ' if c.conv_input else ''}fp32 form"
    if c.ragged:
        for b in range(B):
            one = run.uniform([b], f"{name} (image {b} alone)")
            assert torch.equal(_split_bits(got[b:b + 1]), _split_bits(one)), f"{name}: ragged image {b} differs from the uniform form"


def _split_bits(t):
    return t.contiguous().view(torch.int16)


# -------------------------------------------------------------------------------------------------------------- head + GAP
def _gap_call(x_bf16, B, HW, C, what):
    """mi355_gap on a device bf16 tensor -> (pooled [B][C] fp32, pooled_bf16 [B][C]) on the CPU, guards checked."""
    L = _lib()
    pooled, pbf = _guarded(B * C, torch.float32), _guarded(B * C, torch.bfloat16)
    L.check(L.lib().mi355_gap(x_bf16.data_ptr(), B, HW, C, pooled.data_ptr(), pbf.data_ptr(), L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return _split(pooled, (B, C), what + " pooled"), _split(pbf, (B, C), what + " pooled_bf16")


def _head_gap_call(c, A, W, bias, what):
    L = _lib()
    pooled, pbf = _guarded(c.B * c.ldp, torch.float32), _guarded(c.B * c.ldp, torch.bfloat16)
    path = ctypes.c_int(-1)
    L.check(L.lib().mi355_head_gap_ex(A.data_ptr(), c.lda, W.data_ptr(), c.ldw, bias.data_ptr(), pooled.data_ptr(), pbf.data_ptr(),
                                      c.ldp, c.B, c.HW, c.N, c.K, c.act, ctypes.byref(path), L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert path.value == c.path, f"{what}: ran instantiation {path.value:#x}, expected {c.path:#x} (act | KSMAX << 8)"
    p, pb = _split(pooled, (c.B, c.ldp), what + " pooled"), _split(pbf, (c.B, c.ldp), what + " pooled_bf16")
    assert torch.isnan(p[:, c.N:]).all() and torch.isnan(pb[:, c.N:].float()).all(), f"{what}: wrote into columns N .. ldp"
    assert not torch.isnan(p[:, :c.N]).any(), f"{what}: unwritten pooled values"
    return p[:, :c.N].contiguous(), pb[:, :c.N].contiguous()


@pytest.mark.parametrize("name", list(R.HEAD_CASES))
def test_head_gap_matches_gemm_gap_bits_and_float64(name):
    L = _lib()
    c = R.HEAD_CASES[name]
    d = R.HeadData(c)
    A, W, bias = _bf16_dev(d.A), _bf16_dev(d.W), _dev(d.bias)
    pooled, pbf = _head_gap_call(c, A, W, bias, name)
    np.testing.assert_array_equal(_bits(pbf), R.bf16_bits(pooled.numpy()), err_msg=f"{name}: pooled_bf16 is not bf16(pooled)")
    # (a) the two-kernel path: head conv with a bf16 output, no split-K workspace, then k_gap
    M = c.B * c.HW
    head = _guarded(M * c.N, torch.bfloat16)
    x = L.GemmExArgs(A=A.data_ptr(), lda=c.lda, W=W.data_ptr(), ldw=c.ldw, bias=bias.data_ptr(), out=head.data_ptr(), ldo=c.N, M=M,
                     N=c.N, K=c.K, act=c.act)
    gpath = ctypes.c_int(-1)
    L.check(L.lib().mi355_gemm_bf16_ex(ctypes.byref(x), ctypes.byref(gpath), L.stream_ptr(DEV)))
    pooled2, pbf2 = _gap_call(head, c.B, c.HW, c.N, name + " gemm -> gap")
    hx = _split(head, (c.B, c.HW, c.N), name + " head tensor").float().numpy()
    same = np.array_equal(pooled.numpy().view(np.uint32), pooled2.numpy().view(np.uint32))
    assert same, f"{name}: pooled differs from mi355_gemm_bf16_ex (path {gpath.value:#x}) -> mi355_gap at " \
        f"{np.argwhere(pooled.numpy() != pooled2.numpy())[:4].tolist()}"
    assert torch.equal(_split_bits(pbf), _split_bits(pbf2)), f"{name}: pooled_bf16 differs from the two-kernel path"
    # (b) k_gap on the GPU's own head tensor
    wb = _check(pooled2.numpy(), R.pool(hx), R.pool_tol(hx), name + " (b)", "(image, channel)")
    # (c) against the float64 head that rounds nothing
    ref, tol = d.reference(c)
    wc = _check(pooled.numpy(), ref, tol, name + " (c)", "(image, channel)")
    print(f"head+gap {name:16s} path {c.path:#x} B={c.B} HW={c.HW} N={c.N} K={c.K} lda={c.lda}: (a) bits equal (gemm path "
          f"{gpath.value:#x}), worst |err| / tol (b) {wb:.3f} (c) {wc:.3f}")
    if c.lda > c.K:
        # columns K .. lda-1 of A meet zero weights only: large finite values there must not change a bit
        A2 = d.A.copy()
        A2[:, :, c.K:] = R.bf16_round(np.float32(3.0e4) * (1 + np.arange(c.lda - c.K, dtype=np.float32)))
        p2, _ = _head_gap_call(c, _bf16_dev(A2), W, bias, name + " (A padding filled)")
        assert np.array_equal(p2.numpy().view(np.uint32), pooled.numpy().view(np.uint32)), f"{name}: A's columns K .. lda leak into pooled"


@pytest.mark.parametrize("B,HW,C", R.GAP_CASES)
def test_gap_matches_float64(B, HW, C):
    x = R.gap_data(B, HW, C)
    what = f"gap B={B} HW={HW} C={C}"
    pooled, pbf = _gap_call(_bf16_dev(x), B, HW, C, what)
    assert not torch.isnan(pooled).any(), f"{what}: unwritten pooled values"
    worst = _check(pooled.numpy(), R.pool(x), R.pool_tol(x), what, "(image, channel)")
    np.testing.assert_array_equal(_bits(pbf), R.bf16_bits(pooled.numpy()), err_msg=f"{what}: pooled_bf16 is not bf16(pooled)")
    print(f"{what}: worst |err| / tol = {worst:.3f}")


@pytest.mark.parametrize("B,C,HW,N,has_bias", R.POOL_LINEAR_CASES)
def test_pool_linear_matches_float64(B, C, HW, N, has_bias):
    L = _lib()
    fm, w, bias = R.pool_linear_data(B, C, HW, N, has_bias)
    what = f"pool_linear B={B} C={C} HW={HW} N={N} bias={has_bias}"
    fm_d = _dev(fm)
    w_d = _dev(w) if N else None
    b_d = _dev(bias) if bias is not None else None
    pooled = _guarded(B * C, torch.float32)
    out = _guarded(B * N, torch.float32)
    L.check(L.lib().mi355_pool_linear(fm_d.data_ptr(), B, C, HW, w_d.data_ptr() if N else None, b_d.data_ptr() if b_d is not None else None,
                                      N, out.data_ptr() if N else None, pooled.data_ptr(), L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    p = _split(pooled, (B, C), what + " pooled_out").numpy()
    o = _split(out, (B, N), what + " out").numpy()
    assert not np.isnan(p).any() and not np.isnan(o).any(), f"{what}: unwritten values"
    x = fm.transpose(0, 2, 1)
    wp = _check(p, R.pool(x), R.pool_tol(x), what + " pooled_out", "(image, channel)")
    wo = 0.0
    if N:
        ref, tol = R.pool_linear_out(p, w, bias)
        wo = _check(o, ref, tol, what + " out", "(image, class)")
    print(f"{what}: worst |err| / tol pooled_out {wp:.3f} out {wo:.3f}")


# ------------------------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("B,HW,C,Cvalid", R.LAYOUT_CASES)
def test_layout_kernels_are_exact(B, HW, C, Cvalid):
    L = _lib()
    what = f"layout B={B} HW={HW} C={C} Cvalid={Cvalid}"
    x = R.layout_data(B, HW, C, Cvalid, seed=B + HW + C)                   # [B][Cvalid][HW] fp32
    x_d = _dev(x)
    # nchw -> nhwc: bf16 as torch on the CPU rounds it, exact zeros in the padded channels
    nhwc = _guarded(B * HW * C, torch.bfloat16)
    L.check(L.lib().mi355_nchw_to_nhwc(x_d.data_ptr(), nhwc.data_ptr(), B, HW, C, Cvalid, L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    got = _bits(_split(nhwc, (B, HW, C), what + " nchw_to_nhwc"))
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).transpose(0, 2, 1)
    np.testing.assert_array_equal(R.canon_nan(got[:, :, :Cvalid]), R.canon_nan(want), err_msg=what + ": nchw_to_nhwc values")
    np.testing.assert_array_equal(R.canon_nan(got), R.nchw_to_nhwc(x, B, HW, C, Cvalid), err_msg=what + ": nchw_to_nhwc vs reference")
    assert not got[:, :, Cvalid:].any(), f"{what}: channels Cvalid .. C are not exact zeros"
    # nhwc -> nchw on an input whose channels past Cvalid hold data: out[b][c][p] == float(in[b][p][c]) and nothing else written
    full = R.bf16_bits(R.layout_data(B, HW, C, C, seed=1)).transpose(0, 2, 1).copy()                # [B][HW][C] bits
    in_d = _dev(full.view(np.int16)).view(torch.bfloat16)
    nchw = _guarded(B * Cvalid * HW, torch.float32)
    L.check(L.lib().mi355_nhwc_to_nchw(in_d.data_ptr(), nchw.data_ptr(), B, HW, C, Cvalid, L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    g = _split_nan_ok(nchw, B * Cvalid * HW, what + " nhwc_to_nchw")
    np.testing.assert_array_equal(g.view(np.uint32), R.nhwc_to_nchw(full, B, HW, C, Cvalid).view(np.uint32), err_msg=what + ": nhwc_to_nchw")
    # round trip nhwc -> nchw -> nhwc: the same bits
    back = _guarded(B * HW * C, torch.bfloat16)
    rt_in = _dev(R.nchw_to_nhwc(x, B, HW, C, Cvalid).view(np.int16)).view(torch.bfloat16)
    mid = _guarded(B * Cvalid * HW, torch.float32)
    L.check(L.lib().mi355_nhwc_to_nchw(rt_in.data_ptr(), mid.data_ptr(), B, HW, C, Cvalid, L.stream_ptr(DEV)))
    L.check(L.lib().mi355_nchw_to_nhwc(mid.data_ptr(), back.data_ptr(), B, HW, C, Cvalid, L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(R.canon_nan(_bits(_split(back, (B, HW, C), what + " round trip"))), R.canon_nan(_bits(rt_in.cpu())),
                                  err_msg=what + ": round trip")
    print(f"{what}: exact")


def _split_nan_ok(buf, n, what):
    """fp32 values [n] as numpy; the data itself may hold a NaN, so only the guard is checked for NaNs."""
    t = buf.cpu()
    assert torch.isnan(t[n:]).all(), f"{what}: wrote past the end"
    return t[:n].numpy()
