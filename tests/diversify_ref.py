"""NumPy model of result diversification as include/mi355_retrieval.h defines it (mi355_shortlist_gram / mi355_mmr_select): the
shortlist Gram matrix in float64 of the fp16-rounded rows, and the greedy selection - in fp32 exactly as the kernel is specified
(``select``, the bit-for-bit reference) or in float64 with every pick's winning margin (the end-to-end reference and its
near-ties).  Also the fixture the diversification tests share: ``products``, several shots of every product."""
import numpy as np

ULP = 2.0 ** -24


def gram_tol(D):
    """|fp32 MFMA sum - exact| of two rows of norm <= 1 and D columns: D - 1 additions, each rounding a partial sum of magnitude
    <= 1 by <= 2^-24, whatever their order; the factor covers the fp16-rounded norms, which may exceed 1 by 2^-11 each."""
    return D * ULP * (1 + 2.0 ** -10)


def f16_rows(rows):
    """The operands of the Gram stage: the resident rows rounded to fp16 (round-to-nearest-even; fp16 rows as they lie), float64."""
    return np.asarray(rows).astype(np.float16).astype(np.float64)


def gram(rows, idx):
    """S of one shortlist ``idx`` (L,) or of several (Q, L): float64 dot products of the fp16-rounded ``rows``; 0 wherever either
    slot is a pad (-1, or any index outside the gallery)."""
    idx = np.asarray(idx)
    if idx.ndim == 2:
        return np.stack([gram(rows, i) for i in idx])
    ok = (idx >= 0) & (idx < len(rows))
    x = f16_rows(np.asarray(rows)[np.where(ok, idx, 0)]) * ok[:, None]
    return x @ x.T


def select(rel, idx, S, k, lam, dedup=None, idx_offset=0, dtype=np.float32, follow=None):
    """The greedy selection of one query.  rel (L,), idx (L,) LOCAL rows (< 0: a pad), S (L, L).  With ``dtype=np.float32`` this
    is the kernel's recipe operation for operation: lam32 = fp32(lam), oml = fp32(1) - lam32, v = fp32(lam32 * rel) -
    fp32(oml * m), NaN -> -inf, the eligible slot of greatest v, ties to the lower position, m = S[j] wherever that is greater.
    Returns (cosine scores (k,) fp32, rows + idx_offset (k,) int64, v at pick time (k,) dtype, picks, margins (k,) float64): a
    pick's margin is how far it won by - the gap to the best other eligible slot, and with ``dedup`` also the distance of every
    unpicked slot's m from the threshold - or inf where nothing else was in reach.

    ``follow`` (k,) LOCAL rows, -1 to stop: after each pick the state advances by the row given there instead of the model's own
    choice, so that every position can be judged on its own against another implementation's picks."""
    f = dtype
    rel, idx, S = np.asarray(rel).astype(f), np.asarray(idx), np.asarray(S).astype(f)
    L = len(idx)
    lam32 = f(np.float32(lam))
    oml = f(f(1) - lam32)
    thr = None if dedup is None else f(np.float32(dedup))
    has = idx >= 0
    m, picked = np.zeros(L, f), np.zeros(L, bool)
    vals, out_idx = np.full(k, -np.inf, np.float32), np.full(k, -1, np.int64)
    mmr, margins = np.full(k, -np.inf, f), np.full(k, np.inf)
    count = 0
    for t in range(k):
        elig = has & ~picked
        if thr is not None:
            elig &= m < thr
        if not elig.any():
            break
        with np.errstate(invalid="ignore"):
            v = (lam32 * rel).astype(f) - (oml * m).astype(f)
        v = np.where(np.isnan(v), f(-np.inf), v).astype(f)
        key = np.where(elig, v, f(-np.inf))
        j = int(np.flatnonzero(elig & (key == key[elig].max()))[0])         # the greatest value, the lowest position
        others = elig.copy()
        others[j] = False
        with np.errstate(invalid="ignore"):
            gap = float(v[j]) - float(v[others].max()) if others.any() else np.inf
        if thr is not None and (has & ~picked).any():
            gap = min(gap, float(np.abs(m[has & ~picked].astype(np.float64) - float(thr)).min()))
        margins[t] = gap if gap == gap else 0.0
        vals[t], out_idx[t], mmr[t] = np.float32(rel[j]), idx[j] + idx_offset, v[j]
        count += 1
        if follow is not None:
            if follow[t] < 0:
                break
            j = int(np.flatnonzero(idx == follow[t])[0])
        picked[j] = True
        m = np.where(S[j] > m, S[j], m)
    return vals, out_idx, mmr, count, margins


def near_ties(margins, tol):
    """The positions a float64 reference cannot judge: won by less than twice the Gram tolerance."""
    return np.asarray(margins) < 2 * tol


def products(seed, ncat=20, nprod=10, nshot=10, D=64):
    """``ncat`` categories x ``nprod`` products x ``nshot`` shots of D columns: a category centre is N / sqrt(D), a product centre
    its category's + 0.5 N / sqrt(D), a shot its product's + 0.05 N / sqrt(D), and there is one query per category at its centre
    + 0.2 N / sqrt(D).  Returns (rows (G, D) fp32, category (G,), product (G,), queries (ncat, D) fp32, query category (ncat,))."""
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(D)
    cat = rng.standard_normal((ncat, D)) * s
    prod = cat[:, None, :] + 0.5 * s * rng.standard_normal((ncat, nprod, D))
    shots = prod[:, :, None, :] + 0.05 * s * rng.standard_normal((ncat, nprod, nshot, D))
    rows = shots.reshape(-1, D).astype(np.float32)
    category = np.repeat(np.arange(ncat), nprod * nshot)
    product = np.repeat(np.arange(ncat * nprod), nshot)
    queries = (cat + 0.2 * s * rng.standard_normal((ncat, D))).astype(np.float32)
    return rows, category, product, queries, np.arange(ncat)


def normalized(x):
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def search(rows, queries, L):
    """(scores (Q, L) fp32, rows (Q, L) int64) of a float64 cosine search, descending, ties to the lower row."""
    s = normalized(queries) @ normalized(rows).T
    order = np.argsort(-s, axis=1, kind="stable")[:, :L]
    return np.take_along_axis(s, order, 1).astype(np.float32), order.astype(np.int64)


def distinct(labels, idx):
    """Per query: how many distinct labels its result rows ``idx`` (Q, k) hold (pads left out)."""
    return np.array([len(set(labels[i[i >= 0]].tolist())) for i in np.asarray(idx)])
