"""A float64 NumPy model of the feature-map aggregation (include/mi355_retrieval.h, "Feature-map aggregation"), an independent
restatement of the R-MAC region grid in exact rational arithmetic, and the planted-patch retrieval fixture that shows what the
descriptors are for.  Nothing here imports the package."""
from fractions import Fraction
from math import floor

import numpy as np

EPS_CLAMP = 1e-6


# ---------------------------------------------------------------------------------------------- the region grid
def rmac_regions(H, W, levels=3, overlap=0.4):
    """[(y0, x0, h, w)]: the grid of the issue, the starts in exact fractions, the choice of the extra steps in float64."""
    w = min(H, W)
    costs = [abs((w * w - w * ((max(H, W) - w) / (s - 1))) / (w * w) - overlap) for s in (2, 3, 4, 5, 6, 7)]
    idx = int(np.argmin(np.array(costs, dtype=np.float64)))              # the first minimum
    extra = {"H": idx + 1 if H > W else 0, "W": idx + 1 if W > H else 0}
    out = []
    for l in range(1, levels + 1):
        wl = floor(Fraction(2 * w, l + 1))
        if wl == 0:
            continue
        wl2 = floor(Fraction(wl, 2) - 1)

        def starts(S, d):
            n = l + d
            step = Fraction(S - wl, n - 1) if n > 1 else Fraction(0)
            return [floor(wl2 + i * step) - wl2 for i in range(n)]
        for y in starts(H, extra["H"]):
            for x in starts(W, extra["W"]):
                out.append((y, x, wl, wl))
    return out


# ---------------------------------------------------------------------------------------------- the arithmetic
def normalize_rows(v, eps=1e-6):
    """v / max(|v|, eps) along the last axis."""
    n = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return v / np.maximum(n, eps)


def pool_regions(fm, regions, pool, p=3.0):
    """(B, R, C) float64: every region of every channel pooled.  ``p`` a scalar or a (C,) array."""
    x = np.asarray(fm, dtype=np.float64)
    B, C = x.shape[:2]
    pc = np.broadcast_to(np.asarray(p, dtype=np.float64), (C,)).reshape(1, C, 1)
    out = np.empty((B, len(regions), C))
    for r, (y0, x0, h, w) in enumerate(regions):
        v = x[:, :, y0:y0 + h, x0:x0 + w].reshape(B, C, h * w)
        if pool == "mean":
            out[:, r] = v.sum(axis=2) / (h * w)
        elif pool == "max":
            out[:, r] = v.max(axis=2)
        elif pool == "gem":
            t = np.maximum(v, EPS_CLAMP)
            m = t.max(axis=2, keepdims=True)
            out[:, r] = m[:, :, 0] * (((t / m) ** pc).mean(axis=2)) ** (1.0 / pc[:, :, 0])
        else:
            raise ValueError(pool)
    return out


def crow(fm, normalize=True, eps=1e-6):
    x = np.asarray(fm, dtype=np.float64)
    B, C, H, W = x.shape
    xp = np.maximum(x, 0.0)
    S = xp.sum(axis=1)                                                   # (B, H, W)
    z = np.sqrt((S * S).sum(axis=(1, 2)))
    St = np.zeros_like(S)
    nz = z > 0
    St[nz] = np.sqrt(S[nz] / z[nz, None, None])
    F = (St[:, None] * xp).sum(axis=(2, 3))
    Q = (x > 0).sum(axis=(2, 3)) / float(H * W)
    I = np.zeros_like(Q)
    qs = Q.sum(axis=1, keepdims=True)
    pos = Q > 0
    I[pos] = np.log(np.broadcast_to(qs, Q.shape)[pos] / Q[pos])
    d = I * F
    return normalize_rows(d, eps) if normalize else d


def regional(fm, regions, pool, p=3.0, normalize=True, eps=1e-6):
    v = pool_regions(fm, regions, pool, p)
    return normalize_rows(v, eps) if normalize else v


def summed(v, normalize=True, eps=1e-6):
    s = v.sum(axis=1)
    return normalize_rows(s, eps) if normalize else s


_PRESET = {"spoc": "mean", "mac": "max", "gem": "gem"}


def aggregate(fm, method="gem", p=3.0, levels=3, regions=None, pool=None, normalize=True, eps=1e-6, return_regions=False):
    H, W = fm.shape[2:]
    if method == "crow":
        return crow(fm, normalize, eps)
    if method == "rmac":
        regions = rmac_regions(H, W, levels)
    elif method != "regions":
        regions = [(0, 0, H, W)]
    kind = _PRESET.get(method) or (pool or "max")
    v = regional(fm, [tuple(int(a) for a in r) for r in regions], kind, p, normalize, eps)
    return v if return_regions else summed(v, normalize, eps)


def whitened(fm, regions, pool, matrix, bias, normalize_input, p=3.0, eps=1e-6):
    """The R-MAC regional whitening: regional vectors, normalised; (normalised again when the fit says so - a no-op on unit
    vectors, kept for the zero vector); matrix v + bias, normalised; summed in order; normalised."""
    v = regional(fm, regions, pool, p, True, eps)
    if normalize_input:
        v = normalize_rows(v, eps)
    t = normalize_rows(v @ np.asarray(matrix, dtype=np.float64).T + np.asarray(bias, dtype=np.float64), eps)
    return summed(t, True, eps)


# ---------------------------------------------------------------------------------------------- test inputs
def silu_map(seed, shape, scale=2.0):
    """Signed values through SiLU (so negatives exist), fp32; with more than one image the last image is all zero, and with more
    than one channel, channel 0 is negative everywhere."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * scale
    x = x / (1.0 + np.exp(-x))
    if shape[1] > 1:
        x[:, 0] = -np.abs(x[:, 0]) - 0.05
    if shape[0] > 1:
        x[-1] = 0.0
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------- the planted fixture
CLASSES, PER_CLASS_GALLERY, PER_CLASS_QUERY, FIX_C, FIX_HW = 8, 4, 3, 64, 7
PATCH_AMP, CLUTTER_AMP = 2.5, 1.0


def planted_fixture(seed=7):
    """(gallery maps (32, 64, 7, 7) fp32, gallery labels, query maps (24, 64, 7, 7) fp32, query labels).  Every class has a
    non-negative signature over the 64 channels.  An image of class k carries k's signature, at amplitude 2.5, in a 3 x 3 patch at
    a random place; each of the other 40 positions carries the signature of one of two OTHER classes at amplitude 1.  The mean
    over positions is dominated by the clutter (40 positions against 9); a descriptor that favours large activations is not."""
    rng = np.random.default_rng(seed)
    sig = np.abs(rng.standard_normal((CLASSES, FIX_C))) * (rng.random((CLASSES, FIX_C)) < 0.35)
    sig /= np.sqrt((sig * sig).sum(axis=1, keepdims=True))

    def image(k):
        others = rng.choice([c for c in range(CLASSES) if c != k], size=2, replace=False)
        which = others[rng.integers(0, 2, size=(FIX_HW, FIX_HW))]
        amp = CLUTTER_AMP * (1.0 + 0.1 * rng.standard_normal((FIX_HW, FIX_HW)))
        m = sig[which].transpose(2, 0, 1) * amp[None]
        y, x = rng.integers(0, FIX_HW - 2, size=2)
        pamp = PATCH_AMP * (1.0 + 0.1 * rng.standard_normal((3, 3)))
        m[:, y:y + 3, x:x + 3] = sig[k][:, None, None] * pamp[None]
        m += 0.02 * np.abs(rng.standard_normal(m.shape))
        return m

    gl = np.repeat(np.arange(CLASSES), PER_CLASS_GALLERY)
    ql = np.repeat(np.arange(CLASSES), PER_CLASS_QUERY)
    g = np.stack([image(k) for k in gl]).astype(np.float32)
    q = np.stack([image(k) for k in ql]).astype(np.float32)
    return g, gl, q, ql


def rank_fixture(gd, qd):
    """(top-1 gallery row of every query, the gap between its top-2 scores) for unit descriptors gd (G, D) / qd (Q, D)."""
    s = np.asarray(qd, dtype=np.float64) @ np.asarray(gd, dtype=np.float64).T
    order = np.argsort(-s, axis=1, kind="stable")
    top = np.take_along_axis(s, order[:, :2], axis=1)
    return order[:, 0], top[:, 0] - top[:, 1]


FIXTURE_METHODS = [("spoc", {}), ("mac", {}), ("gem", {}), ("rmac", {}), ("rmac", {"pool": "gem"}), ("crow", {})]
_reference = {}


def fixture_reference(method, kw):
    """(the model's top-1 row of every query, its top-2 gaps, its precision@1) on the planted fixture, computed once."""
    key = (method, tuple(sorted(kw.items())))
    if key not in _reference:
        g, gl, q, ql = planted_fixture()
        top, gap = rank_fixture(aggregate(g, method, **kw), aggregate(q, method, **kw))
        _reference[key] = (top, gap, float((gl[top] == ql).mean()))
    return _reference[key]
