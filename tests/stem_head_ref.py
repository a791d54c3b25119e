"""numpy float64 references, seeded data and cases for the two ends of the conv backbones: the stem in both input forms, the head
conv + global average pool, the pooling kernels and the two layout kernels (tests/test_stem_head_gpu.py compares the kernels
with them on the GPU, tests/test_stem_head_args.py checks the references themselves on the CPU).

Every reference rounds nothing after its inputs: the value is the float64 result on the operands the kernel reads, and `mag` is
the same sum over absolute values (bias included), carried through an activation with its derivative bound.  `mutant` names a
deliberate bug; the CPU test requires each to move some output by more than 10x the tolerance on the case's own data."""
from dataclasses import dataclass

import numpy as np

TOL_REL, TOL_ABS = 2.0 ** -8, 2.0 ** -20        # one bf16 rounding; fp32 accumulation (test_gemm_paths_gpu.py)
TOL_STEM = 2.0 ** -18                           # 28 fp32 terms < 28 * 2^-24 mag < 2^-19 mag, a factor 2 over that (as the depthwise test)
TOL_LINEAR = 2.0 ** -18                         # k_pool_linear: (C / 64 + 7) 2^-24 at the largest C here (1536) = 31 * 2^-24 < 2^-19
U24 = 2.0 ** -24
BN_EPS = 1e-5
GUARD = 256
ACT_NONE, ACT_SILU, ACT_RELU, ACT_RELU6, ACT_GELU, ACT_SIGMOID = range(6)
DERIV = {ACT_NONE: 1.0, ACT_SILU: 1.1, ACT_RELU: 1.0, ACT_RELU6: 1.0}
# include/mi355_retrieval.h (test_path_enums_match_the_header keeps the two in step)
STEM_PATHS = {"F32_LOAD16": 1, "F32_LOAD4": 2, "U8": 3, "CONV_INPUT": 0x100, "RAGGED": 0x200}


# ------------------------------------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even as torch on the CPU; every NaN -> 0x7fc0 (torch's own choice of
    NaN pattern differs between its scalar and vector paths, 0x7fc0 and 0xffff: compare NaNs through canon_nan)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(x)] = 0x7fc0
    return out


def canon_nan(bits):
    """bf16 bit patterns with every NaN replaced by 0x7fc0: a NaN must be a NaN, which one is not specified."""
    bits = np.array(bits, dtype=np.uint16)
    bits[(bits & 0x7fff) > 0x7f80] = 0x7fc0
    return bits


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_to_f32(bf16_bits(x))


def act(z, a):
    if a == ACT_SILU:
        return z / (1.0 + np.exp(-z))
    if a == ACT_RELU:
        return np.maximum(z, 0.0)
    if a == ACT_RELU6:
        return np.clip(z, 0.0, 6.0)
    assert a == ACT_NONE
    return z


def worst(got, ref, tol):
    """(largest |got - ref| / tol, its index)."""
    ratio = np.abs(np.asarray(got, np.float64) - ref) / tol
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), tuple(int(j) for j in np.unravel_index(i, ratio.shape))


# ------------------------------------------------------------------------------------------------------------------ stem
def fold_stem(w_raw, gamma, beta, mean, var):
    """pack_stem's fold in fp32, in the packer's order: s = g / sqrtf(var + eps); w [27][Cout] = bf16(w * s) held in fp32 at
    tap (ky*3 + kx)*3 + ci; bias = beta - mean * s.  w_raw [Cout][3][3][3] (co, ci, ky, kx)."""
    f32 = np.float32
    s = (gamma.astype(f32) / np.sqrt(var.astype(f32) + f32(BN_EPS))).astype(f32)
    wf = bf16_round(w_raw.astype(f32) * s[:, None, None, None])
    bias = (beta.astype(f32) - mean.astype(f32) * s).astype(f32)
    return np.ascontiguousarray(wf.transpose(2, 3, 1, 0).reshape(27, -1)), bias          # (ky, kx, ci) major


def stem(x, w27, bias, a, mutant=None):
    """3x3 stride 2 pad 1 conv + bias + act.  x [B][3][H][W], w27 [27][Cout], bias [Cout] -> (y, mag) [B][Ho][Wo][Cout], float64."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w27, np.float64)
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if mutant == "stride_phase_shifted":                 # column ix + 1 read where ix is due
        x = np.concatenate([x[..., 1:], np.zeros_like(x[..., :1])], -1)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge" if mutant == "pad_reads_edge" else "constant")
    z = np.zeros((B, Ho, Wo, w.shape[1])) + bias.astype(np.float64)
    mag = np.zeros_like(z) + np.abs(bias.astype(np.float64))
    for ky in range(3):
        for kx in range(3):
            for ci in range(3):
                t = (ky * 3 + kx) * 3 + ci
                if mutant == "taps_transposed":
                    t = (kx * 3 + ky) * 3 + ci
                elif mutant == "tap_order_ci_slowest":
                    t = ci * 9 + ky * 3 + kx
                p = xp[:, ci, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][..., None]
                z += p * w[t]
                mag += np.abs(p) * np.abs(w[t])
    return act(z, a), DERIV[a] * mag


def stem_tol(y, mag, extra=0.0):
    return TOL_REL * np.abs(y) + TOL_STEM * (mag + extra)


def preprocess(img, fill, mean, std, mutant=None):
    """SquarePad(fill) -> /255 -> (v - mean) / std with numpy fp32 ops in k_square_pad_normalize's order (one rounding per op:
    bit-exact with the kernel).  img [h][w][3] uint8 -> [3][S][S] fp32."""
    f32 = np.float32
    h, w, _ = img.shape
    S = max(h, w)
    hp, vp = (S - w) // 2, (S - h) // 2
    if mutant == "pad_split_rounded_up":
        hp, vp = (S - w + 1) // 2, (S - h + 1) // 2
    canvas = np.full((S, S, 3), fill, np.uint8)
    canvas[vp:vp + h, hp:hp + w] = img
    v = ((canvas.astype(f32) / f32(255.0)) - np.asarray(mean, f32)) / np.asarray(std, f32)
    if mutant == "border_reads_zero":
        inside = np.zeros((S, S, 1), bool)
        inside[vp:vp + h, hp:hp + w] = True
        v = np.where(inside, v, f32(0.0))
    return np.ascontiguousarray(v.astype(f32).transpose(2, 0, 1))


def conv_input_silu(P, cw, outside=None):
    """SiLU(conv3x3 s1 p1, 3 -> 3, no bias) of P [B][3][S][S] with cw [co][ci][ky][kx], float64 -> (c, mag of the pre-activation).
    outside (mutant): [3] values read outside the square instead of zero; the result then covers the (S + 2)^2 ring too."""
    P = np.asarray(P, np.float64)
    cw = np.asarray(cw, np.float64)
    B, _, S, _ = P.shape
    r = 1 if outside is None else 2
    Pp = np.zeros((B, 3, S + 2 * r, S + 2 * r))
    if outside is not None:
        Pp += np.asarray(outside, np.float64)[None, :, None, None]
    Pp[:, :, r:r + S, r:r + S] = P
    n = S + 2 * (r - 1)
    a = np.zeros((B, 3, n, n))
    mag = np.zeros_like(a)
    for ci in range(3):
        for ky in range(3):
            for kx in range(3):
                p = Pp[:, ci, ky:ky + n, kx:kx + n][:, None]
                wv = cw[:, ci, ky, kx][None, :, None, None]
                a += p * wv
                mag += np.abs(p) * np.abs(wv)
    return act(a, ACT_SILU), mag


def stem_u8(imgs, fill, mean, std, cw, w27, bias, a, mutant=None):
    """The uint8 form on a list of images with one longer side S -> (y, tol) [B][Ho][Ho][Cout]."""
    P = np.stack([preprocess(im, fill, mean, std, mutant) for im in imgs])
    if cw is None:
        y, mag = stem(P, w27, bias, a)
        return y, stem_tol(y, mag)
    if mutant == "conv_input_on_fill_outside":
        f32 = np.float32
        out = ((f32(fill) / f32(255.0)) - np.asarray(mean, f32)) / np.asarray(std, f32)
        c, _ = conv_input_silu(P, cw, outside=out)       # [B][3][S + 2][S + 2]: the ring is what the stem reads as its padding
        S = P.shape[2]
        wd = np.asarray(w27, np.float64)
        Ho = (S - 1) // 2 + 1
        z = np.zeros((len(imgs), Ho, Ho, wd.shape[1])) + bias.astype(np.float64)
        for ky in range(3):
            for kx in range(3):
                for ci in range(3):
                    z += c[:, ci, ky:ky + 2 * Ho:2, kx:kx + 2 * Ho:2][..., None] * wd[(ky * 3 + kx) * 3 + ci]
        return act(z, a), None
    c, mag_a = conv_input_silu(P, cw)
    y, mag = stem(c, w27, bias, a)
    # the conv_input stage's own fp32 error, 2^-18 mag_a through SiLU (1.1), carried through |w_stem| and the stem's activation
    _, carried = stem(DERIV[ACT_SILU] * mag_a, np.abs(w27), np.zeros_like(bias), ACT_NONE)
    return y, stem_tol(y, mag, DERIV[a] * carried)


# ------------------------------------------------------------------------------------------------------------ head + pooling
def head(A, W, bias, a, mutant=None):
    """1x1 conv: A [B][HW][K], W [N][K], bias [N] -> (y, mag) [B][HW][N] float64, nothing rounded."""
    A, W, bias = (np.asarray(t, np.float64) for t in (A, W, bias))
    acc = A @ W.T
    mag = DERIV[a] * (np.abs(A) @ np.abs(W).T + np.abs(bias))
    if mutant == "bias_before_activation":
        return act(acc, a) + bias, mag
    return act(acc + bias, a), mag


def pool(y, mutant=None):
    """Mean over axis 1 of y [B][HW][C], float64."""
    y = np.asarray(y, np.float64)
    HW = y.shape[1]
    if mutant == "pool_drops_last_pixel":
        p = y[:, :-1].sum(1) / HW
    elif mutant == "pool_divides_by_64":
        p = y.sum(1) / 64.0
    elif mutant == "pool_adds_clamped_row":              # rows past HW are clamped copies of the last one
        p = (y.sum(1) + y[:, -1]) / HW
    else:
        p = y.sum(1) / HW
    if mutant == "pool_row_of_neighbour_image":
        B = y.shape[0]
        p = p[[b + 1 if b + 1 < B else b - 1 for b in range(B)]]
    return p


def pool_tol(x):
    """HW sequential fp32 additions, the rounding of 1 / HW and the product: (HW + 2) 2^-24 mean_i |x_i|."""
    x = np.asarray(x, np.float64)
    return (x.shape[1] + 2) * U24 * np.abs(x).mean(1)


def head_gap(A, W, bias, a, mutant=None):
    """Check (c): the pooled head output with nothing rounded -> (ref, tol) [B][N]."""
    y, mag = head(A, W, bias, a, mutant)
    y0, _ = head(A, W, bias, a)
    tol = (TOL_REL * np.abs(y0) + TOL_ABS * mag).mean(1) + pool_tol(y0)
    return pool(y, mutant), tol


POOL_MUTANTS = {
    "pool_drops_last_pixel": lambda B, HW: True,
    "pool_divides_by_64": lambda B, HW: HW != 64,
    "pool_adds_clamped_row": lambda B, HW: HW % 16 != 0,
    "pool_row_of_neighbour_image": lambda B, HW: B > 1,
}


def pool_linear_out(pooled, w, bias):
    """Linear on the given pooled values rounded to bf16, with bf16-rounded weights -> (ref, tol) [B][N]."""
    p = bf16_round(pooled).astype(np.float64)
    wb = bf16_round(w).astype(np.float64)
    ref = p @ wb.T + (0.0 if bias is None else bias.astype(np.float64))
    return ref, TOL_LINEAR * (np.abs(p) @ np.abs(wb).T)


# ------------------------------------------------------------------------------------------------------------------ layout
def nhwc_to_nchw(x_bits, B, HW, C, Cvalid, mutant=None):
    """in [B][HW][C] bf16 bits -> the flat fp32 output buffer of B * Cvalid * HW elements."""
    x = bf16_to_f32(x_bits).reshape(B, HW, C)
    if mutant == "cvalid_ignored":                        # every channel written, at a stride of C: B * C * HW elements
        return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1)
    return np.ascontiguousarray(x[:, :, :Cvalid].transpose(0, 2, 1)).reshape(-1)


def nchw_to_nhwc(x, B, HW, C, Cvalid, mutant=None):
    """in: flat fp32 [B][Cvalid][HW] -> bf16 bits [B][HW][C], zeros for c >= Cvalid."""
    x = np.asarray(x, np.float32).reshape(-1)
    if mutant == "cvalid_ignored":                        # read at a stride of C, nothing zeroed
        src = np.resize(x, B * C * HW).reshape(B, C, HW)
        return bf16_bits(np.ascontiguousarray(src.transpose(0, 2, 1)))
    out = np.zeros((B, HW, C), np.uint16)
    out[:, :, :Cvalid] = bf16_bits(np.ascontiguousarray(x.reshape(B, Cvalid, HW).transpose(0, 2, 1)))
    return out


SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00010000, 0x7f800000, 0xff800000, 0x7fc00000,
                     0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,       # halfway between two bf16 values: even / odd below
                     0x3f808001, 0x3f807fff, 0x7f7fffff, 0xff7fffff,       # just past / just short of halfway; the largest fp32 -> Inf
                     0x7f7f8000, 0x00008000, 0x00018000], np.uint32).view(np.float32)


def layout_data(B, HW, C, Cvalid, seed):
    """fp32 [B][Cvalid][HW]: seeded values, each image with its own scale and offset, with SPECIALS scattered through it."""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((B, Cvalid, HW)) * (0.5 + np.arange(B))[:, None, None] + 0.25 * np.arange(B)[:, None, None]).astype(np.float32)
    flat = x.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size, 3 * SPECIALS.size)]
    flat[pos] = np.resize(SPECIALS, pos.size)
    if flat.size >= 8:
        flat[[0, -1]] = SPECIALS[[14, 8]]                 # first and last element: the largest fp32, a halfway case
    return x


LAYOUT_CASES = [(2, 49, 40, 40), (1, 33, 80, 77), (3, 1, 8, 3), (1, 1025, 8, 8), (2, 64, 32, 32)]      # (B, HW, C, Cvalid)


# ------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class StemCase:
    B: int
    H: int
    W: int
    Cout: int
    act: int

    @property
    def path(self):
        return STEM_PATHS["F32_LOAD16" if self.W % 4 == 0 else "F32_LOAD4"]


STEM_CASES = {
    "one_tile_32x32_c8": StemCase(2, 32, 32, 8, ACT_SILU),
    "load4_33x35_c40": StemCase(3, 33, 35, 40, ACT_SILU),            # Ho 17, Wo 18: the last tile has one row and two columns
    "load16_64x68_c104_lds67504": StemCase(2, 64, 68, 104, ACT_NONE),   # Wo 34: two-column last tile; LDS over 64 KiB
    "cout256_20x20": StemCase(1, 20, 20, 256, ACT_RELU6),
    "map_1x1_c8": StemCase(1, 1, 1, 8, ACT_SILU),
    "map_2x4_c16": StemCase(1, 2, 4, 16, ACT_SILU),
    "load4_18x50_c48": StemCase(2, 18, 50, 48, ACT_SILU),            # W % 4 != 0 and two column tiles
}
STEM_MUTANTS = {
    "pad_reads_edge": lambda c: True,
    "stride_phase_shifted": lambda c: True,
    "taps_transposed": lambda c: c.H > 1 or c.W > 1,       # a 1x1 map only meets the centre tap
    "tap_order_ci_slowest": lambda c: True,
}


def stem_weights(Cout, rng):
    w_raw = (rng.standard_normal((Cout, 3, 3, 3)) * 0.4).astype(np.float32)
    bn = ((rng.rand(Cout) + 0.5).astype(np.float32), (rng.standard_normal(Cout) * 0.2).astype(np.float32),
          (rng.standard_normal(Cout) * 0.1).astype(np.float32), (rng.rand(Cout) + 0.5).astype(np.float32))
    return w_raw, bn


class StemData:
    def __init__(self, c: StemCase):
        rng = np.random.RandomState(3000 + c.B + 7 * c.H + 131 * c.W + 3 * c.Cout)
        b = np.arange(c.B, dtype=np.float64)[:, None, None, None]
        self.x = (rng.standard_normal((c.B, 3, c.H, c.W)) * (0.6 + 0.5 * b) + 0.3 * b + 0.2).astype(np.float32)
        self.w_raw, self.bn = stem_weights(c.Cout, rng)
        self.w, self.bias = fold_stem(self.w_raw, *self.bn)


@dataclass(frozen=True)
class U8Case:
    sizes: tuple                # (h, w) of every image; one longer side
    conv_input: bool
    ragged: bool
    fill: int
    Cout: int
    act: int = ACT_SILU
    mean: tuple = (0.485, 0.456, 0.406)
    std: tuple = (0.229, 0.224, 0.225)

    @property
    def path(self):
        return STEM_PATHS["U8"] | (STEM_PATHS["CONV_INPUT"] if self.conv_input else 0) | (STEM_PATHS["RAGGED"] if self.ragged else 0)

    @property
    def S(self):
        return max(self.sizes[0])


RAGGED_SIZES = ((66, 10), (66, 66), (3, 66), (65, 66))      # Ho = Wo = 33: a one-column last 32-wide tile, a one-row last 8-high tile
_ALT = dict(mean=(0.5, 0.4, 0.3), std=(0.25, 0.5, 0.2))      # a non-default mean / std
U8_CASES = {}
for _ci in (False, True):
    _n = "ci" if _ci else "plain"
    U8_CASES[f"{_n}_64x64"] = U8Case(((64, 64),) * 2, _ci, False, 255, 16)
    U8_CASES[f"{_n}_33x20"] = U8Case(((33, 20),) * 3, _ci, False, 0, 40, **_ALT)
    U8_CASES[f"{_n}_41x70"] = U8Case(((41, 70),) * 2, _ci, False, 37, 24, ACT_NONE if _ci else ACT_SILU)
    U8_CASES[f"{_n}_1x1"] = U8Case(((1, 1),) * 2, _ci, False, 255, 8)
    U8_CASES[f"{_n}_ragged_66"] = U8Case(RAGGED_SIZES, _ci, True, 37 if _ci else 0, 24, **(_ALT if _ci else {}))
U8_MUTANTS = {
    "border_reads_zero": lambda c: any(h != w for h, w in c.sizes),
    "pad_split_rounded_up": lambda c: any((max(h, w) - min(h, w)) % 2 for h, w in c.sizes),
    "conv_input_on_fill_outside": lambda c: c.conv_input,
}


class U8Data:
    def __init__(self, c: U8Case, name: str):
        rng = np.random.RandomState(4000 + sum(map(ord, name)))
        self.imgs = []
        for b, (h, w) in enumerate(c.sizes):                 # every image its own contrast and brightness
            v = rng.rand(h, w, 3) * (90.0 + 50.0 * b) + 20.0 * b + 40.0 * rng.rand(h, 1, 1)
            self.imgs.append(np.clip(v, 0, 255).astype(np.uint8))
        self.cw = (rng.standard_normal((3, 3, 3, 3)) * 0.35).astype(np.float32) if c.conv_input else None
        self.w_raw, self.bn = stem_weights(c.Cout, rng)
        self.w, self.bias = fold_stem(self.w_raw, *self.bn)

    def reference(self, c: U8Case, mutant=None):
        return stem_u8(self.imgs, c.fill, c.mean, c.std, self.cw, self.w, self.bias, c.act, mutant)


@dataclass(frozen=True)
class HeadCase:
    B: int
    HW: int
    N: int
    K: int
    lda: int
    act: int

    @property
    def ldw(self):
        return (self.K + 31) // 32 * 32

    @property
    def Npad(self):
        return (self.N + 15) // 16 * 16

    @property
    def ldp(self):
        return self.N + 8

    @property
    def path(self):
        return self.act | (12 if self.K <= 384 else 16) << 8


HEAD_CASES = {
    "k384_n136": HeadCase(4, 49, 136, 384, 384, ACT_SILU),       # the model's k-depth; the second workgroup has 8 live channels
    "k32_hw64_b5": HeadCase(5, 64, 128, 32, 32, ACT_NONE),       # one k-step, no clamped rows, B % 4 = 1
    "hw1_k40_n8": HeadCase(1, 1, 8, 40, 40, ACT_SILU),           # HW = 1; K % 32 = 8 takes the lda - 8 clamp; Npad = 16
    "hw16_k64": HeadCase(3, 16, 120, 64, 64, ACT_SILU),          # exactly one pixel chunk; two k-steps
    "hw17_k96_n264": HeadCase(2, 17, 264, 96, 96, ACT_NONE),     # one pixel in the second chunk; three k-steps
    "lda400_k392": HeadCase(6, 25, 72, 392, 400, ACT_SILU),      # lda > K
    "k416_ksmax16": HeadCase(4, 49, 128, 416, 416, ACT_SILU),    # KSMAX = 16
    "k512_hw30": HeadCase(2, 30, 64, 512, 512, ACT_NONE),        # K at its limit
}


def pixel_scale(HW):
    """Per-pixel scale: the last pixel stands out, so pooling that loses or repeats it is far outside the tolerance."""
    s = 0.7 + 0.6 * (np.arange(HW) % 3 == 0)
    s[-1] = 5.0
    return s


class HeadData:
    """A [B][HW][lda] (bf16 values, columns K .. lda-1 zero), W [Npad][ldw] zero padded, bias [Npad]."""

    def __init__(self, c: HeadCase):
        rng = np.random.RandomState(5000 + c.B + 3 * c.HW + 7 * c.N + 13 * c.K)
        b = np.arange(c.B, dtype=np.float64)[:, None, None]
        A = np.zeros((c.B, c.HW, c.lda), np.float32)
        A[:, :, :c.K] = (rng.standard_normal((c.B, c.HW, c.K)) * (0.4 + 0.3 * b) + 0.05 * b) * pixel_scale(c.HW)[None, :, None]
        self.A = bf16_round(A)
        W = np.zeros((c.Npad, c.ldw), np.float32)
        W[:c.N, :c.K] = rng.standard_normal((c.N, c.K)) / np.sqrt(c.K)
        self.W = bf16_round(W)
        bias = np.zeros(c.Npad, np.float32)
        bias[:c.N] = rng.standard_normal(c.N) * 0.3
        self.bias = bias

    def reference(self, c: HeadCase, mutant=None):
        return head_gap(self.A[:, :, :c.K], self.W[:c.N, :c.K], self.bias[:c.N], c.act, mutant)


HEAD_MUTANTS = dict(POOL_MUTANTS, bias_before_activation=None)


def head_mutant_applies(mut, c: HeadCase):
    if mut == "bias_before_activation":
        return c.act != ACT_NONE
    return POOL_MUTANTS[mut](c.B, c.HW)


GAP_CASES = [(1, 1, 8), (3, 49, 1536), (33, 144, 8 * 9), (5, 7, 2056)]          # (B, HW, C)


def gap_data(B, HW, C):
    """[B][HW][C] bf16 values, every image its own scale and offset."""
    rng = np.random.RandomState(6000 + B + 3 * HW + 7 * C)
    b = np.arange(B, dtype=np.float64)[:, None, None]
    return bf16_round((rng.standard_normal((B, HW, C)) * (0.5 + 0.25 * b) + 0.1 * b) * pixel_scale(HW)[None, :, None])


POOL_LINEAR_CASES = [(2, 1536, 49, 10, True), (1, 8, 1, 1, True), (3, 200, 16, 7, False), (2, 1000, 9, 0, False)]   # (B, C, HW, N, bias)


def pool_linear_data(B, C, HW, N, has_bias):
    """fm [B][C][HW] fp32, weight [N][C] fp32 (None for N = 0), bias [N] or None."""
    rng = np.random.RandomState(7000 + B + 3 * C + 7 * HW + 11 * N)
    b = np.arange(B, dtype=np.float64)[:, None, None]
    fm = ((rng.standard_normal((B, C, HW)) * (0.5 + 0.25 * b) + 0.1 * b) * pixel_scale(HW)[None, None, :]).astype(np.float32)
    w = (rng.standard_normal((N, C)) / np.sqrt(C)).astype(np.float32) if N else None
    bias = (rng.standard_normal(N) * 0.2).astype(np.float32) if has_bias and N else None
    return fm, w, bias
