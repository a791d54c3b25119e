"""NumPy model of diffusion re-ranking as include/mi355_retrieval.h defines it (mi355_diffusion_graph / _source / _solve): the graph
stage and the conjugate gradients with the freeze rule.  Every function takes the dtype it computes in: float64 is the
reference, ``np.float32`` restates the same steps (S p summed in slot order) and is used only to size the tolerance of the GPU
tests - what fp32 itself costs on those inputs.  Also the fixtures the diffusion tests share: rows on noisy great-circle arcs."""
import numpy as np

FREEZE = 2.0 ** -48
CERT = 5e-5          # tests/test_rerank_gpu.py's CERT, relative to max |f64| of the query


# ---------------------------------------------------------------------------------------------- the index
def power(x, gamma, dtype=np.float64):
    """max(x, 0)^gamma by repeated multiplication, left to right, in ``dtype``."""
    a = np.maximum(np.asarray(x).astype(dtype), dtype(0))
    out = a.copy()
    for _ in range(gamma - 1):
        out = (out * a).astype(dtype)
    return out


def graph(nn, nv, gamma, dtype=np.float64):
    """(cols (G, kd) int32, vals (G, kd), deg (G,)) of the kNN graph nn (G, kd) integers / nv (G, kd) fp32 scores."""
    nn = np.asarray(nn).astype(np.int64)
    G, kd = nn.shape
    a = power(nv, gamma, dtype)
    rows = np.arange(G)[:, None]
    ok = (nn >= 0) & (nn < G)
    j = np.where(ok, nn, 0)
    back = nn[j] == rows[:, :, None]                     # [i][t][u]: nn[j][u] == i
    mutual = ok & back.any(axis=2)
    u = back.argmax(axis=2)                              # the first such slot
    w = np.where(mutual, np.minimum(a, a[j, u]), dtype(0)).astype(dtype)
    deg = np.zeros(G, dtype)
    for t in range(kd):                                  # slot order
        deg = (deg + w[:, t]).astype(dtype)
    with np.errstate(divide="ignore"):
        c = np.where(deg > 0, dtype(1) / np.sqrt(deg, dtype=dtype), dtype(0)).astype(dtype)
    vals = (w * (c[:, None] * c[j]).astype(dtype)).astype(dtype)
    return np.where(mutual, nn, -1).astype(np.int32), vals, deg


def dense(cols, vals):
    """The (G, G) matrix of the index rows."""
    G, kd = cols.shape
    S = np.zeros((G, G), vals.dtype)
    for t in range(kd):
        m = cols[:, t] >= 0
        S[np.nonzero(m)[0], cols[m, t]] += vals[m, t]
    return S


# ---------------------------------------------------------------------------------------------- one query
def source(sv, si, kq, gamma, dtype=np.float64):
    """y (Q, L): max(sv, 0)^gamma on the first kq slots that hold a row."""
    L = si.shape[1]
    return np.where((np.arange(L)[None, :] < kq) & (si >= 0), power(sv, gamma, dtype), dtype(0)).astype(dtype)


def local(cols, vals, rows, dtype=np.float64):
    """(pos (L, kd) local positions, -1 where slot t of shortlist position p is empty, leaves the shortlist or p is a pad;
    val (L, kd) the entries, 0 where pos is -1).  A row that occurs twice is reached at its earlier position."""
    G, kd = cols.shape
    L = len(rows)
    real = (rows >= 0) & (rows < G)
    where = np.full(G, -1, np.int64)
    for p in range(L - 1, -1, -1):
        if real[p]:
            where[rows[p]] = p
    c = cols[np.where(real, rows, 0)]                    # (L, kd)
    pos = np.where(real[:, None] & (c >= 0), where[np.maximum(c, 0)], -1)
    val = np.where(pos >= 0, vals[np.where(real, rows, 0)].astype(dtype), dtype(0)).astype(dtype)
    return pos, val, real


def cg(pos, val, y, alpha, iters, dtype=np.float64):
    """(f (L,), iterations): (I - alpha S_L) f = y by conjugate gradients with the freeze rule, every step in ``dtype``."""
    alpha = dtype(alpha)
    L, kd = pos.shape
    gather = np.maximum(pos, 0)
    f = np.zeros(L, dtype)
    r = y.astype(dtype).copy()
    p = r.copy()
    rs = dtype(np.dot(r, r))
    stop = dtype(FREEZE) * rs
    done = 0
    for _ in range(iters):
        if rs <= stop:
            break
        sp = np.zeros(L, dtype)
        for t in range(kd):                              # slot order
            sp = (sp + val[:, t] * p[gather[:, t]]).astype(dtype)
        ap = (p - alpha * sp).astype(dtype)
        pap = dtype(np.dot(p, ap))
        if not pap > 0:
            break
        step = dtype(rs / pap)
        f = (f + step * p).astype(dtype)
        r = (r - step * ap).astype(dtype)
        rs_new = dtype(np.dot(r, r))
        p = (r + dtype(rs_new / rs) * p).astype(dtype)
        rs = rs_new
        done += 1
    return f, done


def solve(cols, vals, si, y, alpha, iters, dtype=np.float64):
    """(f (Q, L) with -inf on pads, iterations (Q,)) of every query."""
    Q, L = si.shape
    f = np.empty((Q, L), dtype)
    its = np.empty(Q, np.int32)
    for q in range(Q):
        pos, val, real = local(cols, vals, si[q], dtype)
        fq, its[q] = cg(pos, val, np.where(real, y[q], 0), alpha, iters, dtype)
        f[q] = np.where(real, fq, -np.inf)
    return f, its


def direct(cols, vals, rows, y, alpha):
    """np.linalg.solve of the same float64 system (pads solved as isolated rows)."""
    pos, val, _ = local(cols, vals, rows)
    L, kd = pos.shape
    A = np.eye(L)
    for t in range(kd):
        m = pos[:, t] >= 0
        np.subtract.at(A, (np.nonzero(m)[0], pos[m, t]), alpha * val[m, t])
    return np.linalg.solve(A, y.astype(np.float64))


def rank_shortlist(f, si, k):
    """(values, rows, positions) (Q, k): descending f, ties to the earlier position; the pads' -inf sorts last."""
    pos = np.argsort(-f, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(f, pos, 1), np.take_along_axis(si, pos, 1), pos


def close_pairs(f, k):
    """(Q, k) bool: position p of the ranking is NOT certain - an adjacent value (p - 1 or p + 1, of the first k + 1) lies within
    CERT * max |f| of it."""
    s = -np.sort(-f, axis=1, kind="stable")[:, :k + 1]
    scale = np.abs(np.where(np.isfinite(f), f, 0)).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        tight = ~(np.abs(np.diff(s, axis=1)) > CERT * scale)        # (Q, k) between p and p + 1; -inf next to -inf is tight
    out = np.zeros((f.shape[0], k), bool)
    m = tight.shape[1]                                              # k, or L - 1 when the ranking ends at k = L
    out[:, :min(m, k)] |= tight[:, :k]
    out[:, 1:min(m + 1, k)] |= tight[:, :min(m + 1, k) - 1]
    return out


# ---------------------------------------------------------------------------------------------- searches and fixtures
def normalise(x):
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def knn(q, g, k, exclude=None):
    """(values fp32, rows) (Q, k) of the float64 cosine search: descending, ties to the lower row; ``exclude`` one row per query."""
    s = normalise(q) @ normalise(g).T
    if exclude is not None:
        s[np.arange(len(s)), exclude] = -np.inf
    idx = np.argsort(-s, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(s, idx, 1).astype(np.float32), idx


def arcs(narcs=12, per=40, D=32, noise=0.03, span=2.2, seed=0):
    """(rows (narcs * per, D) fp32, labels): ``per`` points evenly along ``span`` radians of a random great circle per arc, each
    with Gaussian noise of that standard deviation per coordinate.  Row a * per is the start of arc a, a * per + per - 1 its end."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(narcs):
        uv, _ = np.linalg.qr(rng.standard_normal((D, 2)))
        th = np.linspace(0.0, span, per)
        out.append(np.cos(th)[:, None] * uv[:, 0] + np.sin(th)[:, None] * uv[:, 1] + noise * rng.standard_normal((per, D)))
    return np.concatenate(out).astype(np.float32), np.repeat(np.arange(narcs), per)


def arc_queries(rows, narcs, per, nq, noise=0.03, seed=1):
    """(queries (nq, D) fp32, own rows (nq,), labels (nq,)): the arc ends in turn (start of arc 0, end of arc 0, start of arc 1 ...),
    each perturbed by fresh noise; ``own`` is the row a query was made from (to be excluded)."""
    rng = np.random.default_rng(seed)
    ends = np.array([a * per + e * (per - 1) for a in range(narcs) for e in (0, 1)])
    own = ends[np.arange(nq) % len(ends)]
    q = rows[own].astype(np.float64) + noise * rng.standard_normal((nq, rows.shape[1]))
    return q.astype(np.float32), own, own // per


def r_precision(ranked, labels, qlabels, own):
    """The mean share of relevant rows (same label, not the query's own row) among each query's first R results, R the number
    of relevant rows."""
    out = []
    for q in range(len(ranked)):
        rel = (labels == qlabels[q])
        rel[own[q]] = False
        R = int(rel.sum())
        top = ranked[q][:R]
        out.append(rel[top[top >= 0]].sum() / R)
    return float(np.mean(out))


def diffuse(g, q, k, kd, kq, alpha, gamma, iters, L, exclude=None):
    """The whole pipeline in float64 on fp32 inputs: (f-values, rows) (Q, k)."""
    G = len(g)
    nv, nn = knn(g, g, kd, np.arange(G))
    cols, vals, _ = graph(nn, nv, gamma)
    sv, si = knn(q, g, L, exclude)
    f, _ = solve(cols, vals, si, source(sv, si, kq, gamma), alpha, iters)
    v, i, _ = rank_shortlist(f, si, k)
    return v, i
