"""NumPy reference of the row norm and the row-wise ops of rank.hip: ``mi355_l2_normalize_rows`` (``row_inv_norm``,
rank_common.h), ``mi355_pair_cosine``, ``mi355_contrastive_loss`` and ``mi355_cosine_embedding_loss``.

Each op has three parts here:

* its float64 DEFINITION, as include/mi355_retrieval.h and the kernel comments state it.  The scalar arguments an entry takes
  as ``float`` (eps, label, margin) enter as their fp32 values: that is what the kernel is given;
* a forward-error BOUND for an fp32 kernel, counted in fp32 roundings (U = 2^-24 each, round to nearest; first order in U -
  tests/test_rowops_ref.py keeps the fp32 restatement within HALF of every bound, which leaves the second-order terms room);
* an fp32 RESTATEMENT in the kernel's own order (``*32``): lane l of the wave adds elements l, l + 64, ... (or the float4
  chunks l, l + 64, ... of the vector path), six xor-shuffle levels add the 64 lanes, a loss adds rows w, w + 16, ... in wave w
  and then the 16 partials in wave order.  Every product and every add is rounded (NumPy fp32); hipcc contracts some pairs
  into one fma, which only removes roundings.  The restatement sizes nothing on the GPU: the CPU test uses it to show that
  the bounds are neither vacuous nor below what fp32 itself costs.

How a sum is counted.  A lane adds n = ceil(dim / 64) rounded products: a summand passes one rounding as a product and at
most n - 1 as part of a running sum, then 6 more in the wave sum - n + 6 in all (``sum_roundings``).  For non-negative
summands the computed sum is off by at most that count times U, relative to the sum; for a dot product of either sign it is
off by that count times U times sum |a_i b_i|.

The float4 order of ``row_inv_norm`` (dim % 4 == 0, 16-byte aligned rows): a lane first adds the four squares of a chunk,
((x^2 + y^2) + z^2) + w^2 - 4 roundings on the first square - then adds ceil(dim / 256) chunk sums, then the wave sum, whose
levels that only meet the zeros of idle lanes are exact: 4 + ceil(dim / 256) - 1 + min(6, ceil(log2(dim / 4))).  That is at
most n + 6 for every dim but 36 ... 192 (``vec_sum_roundings``), where it is n + 7: the bound below keeps the count n + 6
for both orders - half a rounding less than the float4 worst case at those dims, against an observed error of about 3 U at
most over the dims from 1 to 6000 in either order (a worst case needs every rounding to err fully and in one direction).

This file also holds the shapes and the seeded inputs that the CPU test and tests/test_rowops_gpu.py share."""
import numpy as np

U = 2.0 ** -24
WAVE, LEVELS, LOSS_WAVES = 64, 6, 16
F32 = np.float32


def chunks(dim):
    """Elements per lane: ceil(dim / 64)."""
    return -(-int(dim) // WAVE)


def sum_roundings(dim):
    """Roundings a summand passes in the lane-strided sum of ``dim`` products: n + 6."""
    return chunks(dim) + LEVELS


def vec_sum_roundings(dim):
    """The same count for the float4 order of ``row_inv_norm`` (dim % 4 == 0); see the module docstring."""
    units = dim // 4
    levels = min(LEVELS, int(np.ceil(np.log2(units))) if units > 1 else 0)
    return 4 + (chunks(units) - 1) + levels


# ------------------------------------------------------------------------------------------------ shapes the tests share
NORM_DIMS = (1, 2, 3, 4, 5, 63, 64, 65, 252, 255, 256, 257, 260, 1536, 6000)
NORM_ROWS = (1, 3, 4, 5, 9)                     # k_row_norm and k_pair_cosine: four rows per block
OP_DIMS = (1, 63, 64, 65, 256, 1536)
PAIR_ROWS = (1, 3, 4, 5, 1000)
LOSS_ROWS = (1, 15, 16, 17, 33, 1000)           # the losses: wave w owns rows w, w + 16, ...
CL_LABELS, CL_MARGINS = (0.0, 1.0, 0.3), (0.0, 0.5, 2.0)
CE_TARGETS, CE_MARGINS = (1.0, -1.0), (0.0, 0.5)
EPS = 1e-6


def norm_case(rows, dim):
    """(rows, dim) fp32 normal rows whose norms spread over four decades, all far above eps."""
    rng = np.random.default_rng(100000 + 16 * dim + rows)
    x = rng.standard_normal((rows, dim)) * 10.0 ** rng.uniform(-2, 2, (rows, 1))
    x = np.where(np.abs(x) < 1e-3, 1e-3, x)                      # dim = 1: a row is its one element
    return x.astype(F32)


def pair_case(rows, dim):
    """Two (rows, dim) fp32 batches: b correlates with a (cosines spread over (-1, 1)), norms differ per row."""
    rng = np.random.default_rng(200000 + 16 * dim + rows)
    a = rng.standard_normal((rows, dim))
    mix = rng.uniform(-1, 1, (rows, 1))
    b = mix * a + (1 - np.abs(mix)) * rng.standard_normal((rows, dim))
    a *= 10.0 ** rng.uniform(-1, 1, (rows, 1))
    b *= 10.0 ** rng.uniform(-1, 1, (rows, 1))
    return a.astype(F32), b.astype(F32)


def contrastive_case(rows, dim):
    """Two (rows, dim) fp32 batches whose row distances |f2 - f1| lie around 0.05 ... 1.5: a margin of 0.5 is active on some
    rows and inactive on others (rows >= 15), a margin of 2 is active on all, a margin of 0 on none."""
    rng = np.random.default_rng(300000 + 16 * dim + rows)
    f1 = rng.standard_normal((rows, dim))
    diff = rng.standard_normal((rows, dim))
    diff *= rng.uniform(0.05, 1.5, (rows, 1)) / np.sqrt((diff * diff).sum(1, keepdims=True))
    return f1.astype(F32), (f1 + diff).astype(F32)


def cosine_case(Q, G=300, D=256, seed=1):
    """Queries (Q, D) and gallery (G, D), fp32: five shared directions plus a tenth of full-rank noise, so that the cosines
    spread over most of (-1, 1) - on plain random rows at D = 256 they crowd into +-0.2 and four in ten queries have two
    of their 151 best scores closer than the 2e-6 that certifies an index.  Row norms spread over two decades."""
    rng = np.random.default_rng(400000 + 1000 * seed + Q)
    basis = rng.standard_normal((5, D))
    q = rng.standard_normal((Q, 5)) @ basis + 0.1 * np.sqrt(5.0) * rng.standard_normal((Q, D))
    g = rng.standard_normal((G, 5)) @ basis + 0.1 * np.sqrt(5.0) * rng.standard_normal((G, D))
    q *= 10.0 ** rng.uniform(-1, 1, (Q, 1))
    g *= 10.0 ** rng.uniform(-1, 1, (G, 1))
    return q.astype(F32), g.astype(F32)


COSINE_QS = (3, 70)
COSINE_KS = (3, 150)
CERT_GAP = 2e-6                                 # an index is asserted where the float64 gaps of its row exceed this
SCORE_BOUND = 1e-6                              # test_split_loop_on_ragged_shapes_and_wide_dynamic_range's bound on a score


def cosine64(q, g, eps=EPS, unit_gallery=False):
    """(Q, G) float64 cosines; ``unit_gallery``: the gallery rows are taken as they are (gallery_is_normalized)."""
    gn = np.asarray(g, np.float64) if unit_gallery else normalize(g, eps)
    return normalize(q, eps) @ gn.T


def topk64(s, k):
    """(order (Q, k + 1) by descending score with ties to the lower index, their scores, certified (Q,)): a row is
    certified when consecutive scores among its first k + 1 are more than CERT_GAP apart."""
    order = np.argsort(-s, axis=1, kind="stable")[:, : k + 1]
    srt = np.take_along_axis(s, order, 1)
    cert = (srt[:, :-1] - srt[:, 1:]).min(1) > CERT_GAP if srt.shape[1] > 1 else np.ones(len(s), bool)
    return order, srt, cert


# ------------------------------------------------------------------------------------------------ the lane and wave order
def _lane_sums(p):
    """(R, 64) fp32: lane l's running sum of units l, l + 64, ... of p (R, units) fp32, in that order."""
    R, units = p.shape
    n = chunks(units)
    pad = np.zeros((R, n * WAVE), F32)
    pad[:, :units] = p
    t = pad.reshape(R, n, WAVE)
    acc = np.zeros((R, WAVE), F32)
    for i in range(n):
        acc = acc + t[:, i]                                      # (the first add, to +0, is exact)
    return acc


def _wave_sum(acc):
    """wave_sum of common.h: v += shfl_xor(v, o) for o = 32 ... 1; every lane ends with the same value."""
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


def _dot32(a, b):
    """The scalar order: lane-strided sum of the rounded products a_i * b_i, then the wave sum."""
    return _wave_sum(_lane_sums(a * b))


def _sumsq32_vec(x):
    """The float4 order of row_inv_norm: ((x^2 + y^2) + z^2) + w^2 per chunk, chunks lane-strided, then the wave sum."""
    q = x * x
    return _wave_sum(_lane_sums(((q[:, 0::4] + q[:, 1::4]) + q[:, 2::4]) + q[:, 3::4]))


def _block_sum32(per_row, mean):
    """The losses' reduction: wave w adds rows w, w + 16, ... in that order, thread 0 adds the 16 partials in wave order."""
    rows = len(per_row)
    m = -(-rows // LOSS_WAVES)
    pad = np.zeros(m * LOSS_WAVES, F32)
    pad[:rows] = per_row
    t = pad.reshape(m, LOSS_WAVES)
    acc = np.zeros(LOSS_WAVES, F32)
    for i in range(m):
        acc = acc + t[i]
    s = F32(0)
    for w in range(LOSS_WAVES):
        s = F32(s + acc[w])
    return F32(s / F32(rows)) if mean else s


def _block_sum_bound(per_row, per_row_bound, mean):
    """Bound of that reduction for non-negative losses: the rows' own errors, ceil(rows / 16) + 16 adds, the division."""
    rows = len(per_row)
    total = float(np.sum(per_row + per_row_bound))
    b = float(np.sum(per_row_bound)) + (-(-rows // LOSS_WAVES) + LOSS_WAVES) * U * total
    return (b + U * total) / rows if mean else b


# ------------------------------------------------------------------------------------------------ l2_normalize_rows
def normalize(x, eps=EPS):
    """x / max(|x|_2, eps), float64, row by row (eps as its fp32 value)."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), float(F32(eps)))


def normalize_bound(dim):
    """Per-ELEMENT relative error of an fp32 row normalisation, for rows whose true norm is at least eps and whose elements
    and squares are normal numbers: the sum of squares is off by (n + 6) U relative (``sum_roundings``), its square root by
    half of that; then the square root's own rounding, the reciprocal's and the multiplication's:
    ((n + 6) / 2 + 3) U.  A row below eps costs the reciprocal of eps and the multiplication only (2 U)."""
    return (sum_roundings(dim) / 2.0 + 3.0) * U


def normalize32(x, eps=EPS, vec=False):
    """row_inv_norm and the scaling of k_row_norm in fp32; ``vec``: the float4 order (dim % 4 == 0)."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ss = _sumsq32_vec(x) if vec else _dot32(x, x)
        r = F32(1) / np.maximum(np.sqrt(ss), F32(eps))
        return x * r[:, None]


# ------------------------------------------------------------------------------------------------ pair_cosine
def pair_cosine(a, b, eps=EPS):
    """a.b / (max(|a|, eps) * max(|b|, eps)) per row, float64: each norm is clamped on its own."""
    a, b, e = np.asarray(a, np.float64), np.asarray(b, np.float64), float(F32(eps))
    with np.errstate(invalid="ignore", over="ignore"):
        return (a * b).sum(1) / (np.maximum(np.sqrt((a * a).sum(1)), e) * np.maximum(np.sqrt((b * b).sum(1)), e))


def pair_cosine_bound(a, b, eps=EPS):
    """Per-row ABSOLUTE error.  With c the cosine, da, db the clamped norms and A = sum |a_i b_i| / (da db) (|c| <= A <= 1):
    the dot product is off by (n + 6) U sum |a_i b_i|, i.e. (n + 6) U A in the quotient; each norm by ((n + 6) / 2 + 1) U
    relative (half its sum's error, and the square root; a clamped norm is exact), their product by one rounding more and the
    division by another: (n + 6 + 4) U |c|.  Together ((n + 6) A + (n + 10) |c|) U.  Two zero rows give exactly 0."""
    a, b, e = np.asarray(a, np.float64), np.asarray(b, np.float64), float(F32(eps))
    s = sum_roundings(a.shape[1])
    den = np.maximum(np.sqrt((a * a).sum(1)), e) * np.maximum(np.sqrt((b * b).sum(1)), e)
    A = np.abs(a * b).sum(1) / den
    return (s * A + (s + 4) * np.abs(pair_cosine(a, b, eps))) * U


def pair_cosine32(a, b, eps=EPS):
    """k_pair_cosine in fp32 (scalar loads only)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        xx, yy, xy = _dot32(a, a), _dot32(b, b), _dot32(a, b)
        return xy / (np.maximum(np.sqrt(xx), F32(eps)) * np.maximum(np.sqrt(yy), F32(eps)))


# ------------------------------------------------------------------------------------------------ ContrastiveLoss
CL_SQRT_EPS = 1e-9


def _reduce64(per_row, mean):
    return float(per_row.mean() if mean else per_row.sum())


def contrastive(f1, f2, label, margin):
    """(per-row losses, their sum, their mean), float64: 0.5 (label d + (1 - label) relu(margin - sqrt(d + 1e-9))^2) with
    d = sum (f2 - f1)^2 (utils/contrastive_loss.py of the reference; label and margin as their fp32 values)."""
    t = np.asarray(f2, np.float64) - np.asarray(f1, np.float64)
    lam, m = float(F32(label)), float(F32(margin))
    d = (t * t).sum(1)
    h = np.maximum(m - np.sqrt(d + CL_SQRT_EPS), 0.0)
    per = 0.5 * (lam * d + (1.0 - lam) * h * h)
    return per, float(per.sum()), float(per.mean())


def contrastive_bound(f1, f2, label, margin):
    """(per-row, sum, mean) ABSOLUTE errors, for 0 <= label <= 1 (every summand is non-negative).
    d: a difference is rounded once and squared (2 roundings on the square), then the product and the sum: (n + 8) U relative.
    label d: one more.  s = sqrt(d + 1e-9): the constant is an fp32 constant and the add rounds, (n + 10) U under the root,
    half of it outside, and the root's rounding: ((n + 10) / 2 + 1) U relative.  h = relu(margin - s) is off by that times s,
    and by U |margin - s| for the subtraction (relu is 1-Lipschitz): dh.  (1 - label) h h: three roundings,
    and (h + dh)^2 - h^2 = 2 h dh + dh^2.  The sum of the two terms rounds once; the factor 0.5 is exact.
    The reduction: ``_block_sum_bound``."""
    t = np.asarray(f2, np.float64) - np.asarray(f1, np.float64)
    n = chunks(t.shape[1])
    lam, m = float(F32(label)), float(F32(margin))
    d = (t * t).sum(1)
    s = np.sqrt(d + CL_SQRT_EPS)
    h = np.maximum(m - s, 0.0)
    t1, t2 = lam * d, (1.0 - lam) * h * h
    dh = s * ((n + 10) / 2.0 + 1.0) * U + np.abs(m - s) * U
    e1 = t1 * (n + 9) * U
    e2 = (1.0 - lam) * (2.0 * h * dh + dh * dh + 3.0 * U * (h + dh) ** 2)
    per_b = 0.5 * (e1 + e2 + U * (t1 + t2 + e1 + e2))
    per = 0.5 * (t1 + t2)
    return per_b, _block_sum_bound(per, per_b, False), _block_sum_bound(per, per_b, True)


def contrastive32(f1, f2, label, margin):
    """k_contrastive in fp32: (per-row losses, sum, mean)."""
    f1, f2 = np.asarray(f1, F32), np.asarray(f2, F32)
    lam, m = F32(label), F32(margin)
    t = f2 - f1
    d = _dot32(t, t)
    h = np.maximum(m - np.sqrt(d + F32(CL_SQRT_EPS)), F32(0))
    per = F32(0.5) * (lam * d + (F32(1) - lam) * h * h)
    return per, _block_sum32(per, False), _block_sum32(per, True)


# ------------------------------------------------------------------------------------------------ CosineEmbeddingLoss
CE_EPS = 1e-12


def _ce_cos(x1, x2):
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    return (x1 * x2).sum(1) / np.sqrt(((x1 * x1).sum(1) + CE_EPS) * ((x2 * x2).sum(1) + CE_EPS))


def cosine_embedding(x1, x2, target, margin):
    """(per-row losses, sum, mean), float64: cos = xy / sqrt((xx + 1e-12)(yy + 1e-12)) (ATen's cosine_embedding_loss), then
    1 - cos for target +1 and max(0, cos - margin) for target -1 (margin as its fp32 value)."""
    c = _ce_cos(x1, x2)
    per = 1.0 - c if target > 0 else np.maximum(c - float(F32(margin)), 0.0)
    return per, float(per.sum()), float(per.mean())


def cosine_embedding_bound(x1, x2, target, margin):
    """(per-row, sum, mean) ABSOLUTE errors.  With A = sum |x_i y_i| / sqrt((xx + 1e-12)(yy + 1e-12)) <= 1: the dot product
    costs (n + 6) U A in the quotient.  xx + 1e-12: n + 6, the fp32 constant and the add, (n + 8) U relative; the product of
    the two one rounding more, 2 n + 17; its root half of that and its own rounding, n + 9.5; the division one more:
    (n + 10.5) U |cos|.  1 - cos, or the subtraction of the margin, rounds once more (max is 1-Lipschitz).  The losses are
    non-negative: the reduction is ``_block_sum_bound``."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    n = chunks(x1.shape[1])
    c = _ce_cos(x1, x2)
    A = np.abs(x1 * x2).sum(1) / np.sqrt(((x1 * x1).sum(1) + CE_EPS) * ((x2 * x2).sum(1) + CE_EPS))
    dc = ((n + 6) * A + (n + 10.5) * np.abs(c)) * U
    per = 1.0 - c if target > 0 else np.maximum(c - float(F32(margin)), 0.0)
    per_b = dc + U * (np.abs(1.0 - c) if target > 0 else np.abs(c - float(F32(margin))))
    return per_b, _block_sum_bound(per, per_b, False), _block_sum_bound(per, per_b, True)


def cosine_embedding32(x1, x2, target, margin):
    """k_cos_embedding_loss in fp32: (per-row losses, sum, mean)."""
    x1, x2 = np.asarray(x1, F32), np.asarray(x2, F32)
    xx, yy, xy = _dot32(x1, x1), _dot32(x2, x2), _dot32(x1, x2)
    c = xy / np.sqrt((xx + F32(CE_EPS)) * (yy + F32(CE_EPS)))
    per = F32(1) - c if target > 0 else np.maximum(c - F32(margin), F32(0))
    return per, _block_sum32(per, False), _block_sum32(per, True)
