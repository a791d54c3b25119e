"""Float64 numpy reference of spherical k-means and the clustering scores (tests only)."""
import numpy as np


def normalise(x, eps=1e-6):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), eps)


def scores(x, c, eps=1e-6, unit_rows=False):
    """(N, K) float64 cosines of the rows of x to the rows of c.  unit_rows: x holds the stored rows of a resident gallery,
    which a search takes as they are (fp16 rows are unit only up to their rounding)."""
    return (np.asarray(x, np.float64) if unit_rows else normalise(x, eps)) @ normalise(c, eps).T


def assign(x, c, eps=1e-6, unit_rows=False):
    """(assign (N,) int64, score (N,) f64, gap (N,) f64): arg-max with the lowest index on ties, the best score and
    best minus second best (inf with one centroid)."""
    s = scores(x, c, eps, unit_rows)
    a = s.argmax(axis=1)                      # numpy: the first maximum
    best = s[np.arange(s.shape[0]), a]
    if s.shape[1] > 1:
        t = s.copy()
        t[np.arange(s.shape[0]), a] = -np.inf
        gap = best - t.max(axis=1)
    else:
        gap = np.full(s.shape[0], np.inf)
    return a.astype(np.int64), best, gap


def update(xn, a, K, previous, eps=1e-6):
    """(centroids (K, D) f64, counts (K,), kept (K,) bool) from NORMALISED rows xn: the sequential float64 sum of each
    cluster's rows in ascending row order, normalised; no member or |sum| < eps keeps previous."""
    xn = np.asarray(xn, np.float64)
    out = np.array(previous, np.float64, copy=True)
    counts = np.bincount(a, minlength=K).astype(np.int64)
    kept = np.ones(K, bool)
    for k in range(K):
        rows = np.nonzero(a == k)[0]
        if rows.size == 0:
            continue
        s = np.zeros(xn.shape[1])
        for r in rows:
            s += xn[r]
        n = np.sqrt((s * s).sum())
        if n < eps:
            continue
        out[k] = s / n
        kept[k] = False
    return out, counts, kept


def kmeans(x, init, iters=20, eps=1e-6):
    """The loop: assign, stop if nothing changed, else update.  Returns dict(centroids, assignments, scores, iterations =
    assignment passes run, converged, min_gap over every pass, objectives per pass)."""
    xn = normalise(x, eps)
    c = np.asarray(init, np.float64)
    K = c.shape[0]
    last, passes, updates, converged, min_gap, obj = None, 0, 0, False, np.inf, []
    while True:
        a, s, gap = assign(x, c, eps)
        passes += 1
        min_gap = min(min_gap, float(gap.min()))
        obj.append(float(s.mean()))
        if last is not None and (a == last).all():
            converged = True
            break
        if updates == iters:
            break
        c, _, _ = update(xn, a, K, c, eps)
        updates += 1
        last = a
    return dict(centroids=c, assignments=a, scores=s, iterations=passes, converged=converged, min_gap=min_gap,
                objectives=obj)


def planted(seed, N, D, K, noise):
    """The planted input of the issue: (x (N, D) f32, labels (N,), init = rows 0..K-1)."""
    rng = np.random.default_rng(seed)
    c = normalise(rng.standard_normal((K, D)))
    lab = np.arange(N) % K
    x = (c[lab] + noise * rng.standard_normal((N, D))).astype(np.float32)
    return x, lab.astype(np.int64), x[:K].copy()


PLANTED = [(0, 2000, 70, 9, 0.05), (0, 1000, 1536, 5, 0.08), (3, 1000, 1536, 5, 0.08)]   # (seed, N, D, K, noise)


def contingency(a, b):
    """(table, a_values, b_values): labels made dense by sorted unique value."""
    av, ai = np.unique(a, return_inverse=True)
    bv, bi = np.unique(b, return_inverse=True)
    t = np.zeros((av.size, bv.size), np.int64)
    np.add.at(t, (ai, bi), 1)
    return t, av, bv


def metrics_from_table(t):
    t = np.asarray(t, np.float64)
    N = t.sum()
    a, b = t.sum(1), t.sum(0)
    info = 0.0
    for i in range(t.shape[0]):
        for j in range(t.shape[1]):
            if t[i, j] > 0:
                info += t[i, j] / N * np.log(N * t[i, j] / (a[i] * b[j]))
    ha = -sum(v / N * np.log(v / N) for v in a if v > 0)
    hb = -sum(v / N * np.log(v / N) for v in b if v > 0)
    c2 = lambda v: v * (v - 1.0) / 2.0
    tp, pa, pb = c2(t).sum(), c2(a).sum(), c2(b).sum()
    p = tp / pa if pa > 0 else 1.0
    r = tp / pb if pb > 0 else 1.0
    return {"nmi": 2.0 * info / (ha + hb) if ha + hb > 0 else 1.0, "purity": t.max(axis=1).sum() / N,
            "f1": 2.0 * p * r / (p + r) if p + r > 0 else 0.0, "precision": p, "recall": r,
            "n_clusters": int((a > 0).sum()), "n_classes": int((b > 0).sum()), "info": info}


def metrics(assignments, labels):
    return metrics_from_table(contingency(assignments, labels)[0])
