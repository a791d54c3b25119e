"""NumPy model of ``dbscan`` / ``connected_components`` (imageretrievalresearch_amd/cluster.py) and the fixtures of their tests.

The model takes the DIRECTED hits of a self-join as CSR - ``indices[offsets[i]:offsets[i + 1]]`` are the rows j with
``hit(i, j)``, ``scores`` the score of query i against row j - and restates the specification with a breadth-first search and
Python comparisons, nothing shared with the GPU code:

* ``degree[i]`` = the number of hits of row i (the row itself counts); core = ``degree >= min_samples``;
* core rows i, j are linked when ``hit(i, j)`` or ``hit(j, i)``; a cluster is a connected component of the core rows, its root
  the smallest of them; clusters are numbered by ascending root;
* a non-core row b collects ``(score(i, b), i)`` for core i with ``hit(i, b)`` and ``(score(b, i), i)`` for core i with
  ``hit(b, i)`` and joins the cluster of the candidate with the highest score, equal scores (as floats: -0 equals +0, the
  order of the library's integer keys) going to the lowest core row; without a candidate it is noise (-1).
"""
import numpy as np

N_ROWS = 300
CHAIN_T, CHAIN_MIN = 0.9925, 3
STAR_T, STAR_MIN = 0.7, 4


def model(n, offsets, indices, scores, min_samples):
    """dict(labels, core, degree, roots, counts) of the directed hits (CSR) under ``min_samples``."""
    offsets, indices, scores = np.asarray(offsets), np.asarray(indices), np.asarray(scores)
    assert offsets.shape == (n + 1,) and indices.shape == scores.shape == (int(offsets[-1]),)
    assert not np.isnan(scores).any()                     # a NaN score is never a hit
    degree = np.diff(offsets).astype(np.int64)
    core = degree >= min_samples
    nbr = [set() for _ in range(n)]                       # undirected links between core rows
    best = {}                                             # non-core row -> (score, -core row), the greatest
    for i in range(n):
        for p in range(int(offsets[i]), int(offsets[i + 1])):
            j, s = int(indices[p]), scores[p]
            if i == j:
                continue
            if core[i] and core[j]:
                nbr[i].add(j)
                nbr[j].add(i)
            elif core[i] != core[j]:
                c, b = (i, j) if core[i] else (j, i)
                key = (s + 0.0, -c)
                if b not in best or key > best[b]:
                    best[b] = key
    root = np.full(n, -1, dtype=np.int64)
    for i in range(n):                                    # ascending: the first row of a component is its smallest
        if core[i] and root[i] < 0:
            root[i] = i
            todo = [i]
            while todo:
                for j in nbr[todo.pop()]:
                    if root[j] < 0:
                        root[j] = i
                        todo.append(j)
    for b, (_, negc) in best.items():
        root[b] = root[-negc]
    roots = np.unique(root[root >= 0])
    labels = np.full(n, -1, dtype=np.int64)
    labels[root >= 0] = np.searchsorted(roots, root[root >= 0])
    counts = np.bincount(labels[labels >= 0], minlength=len(roots)).astype(np.int64)
    return {"labels": labels, "core": core, "degree": degree, "roots": roots.astype(np.int64), "counts": counts}


def csr_of(scores, threshold):
    """The directed hits ``scores[i, j] >= threshold`` of a dense (n, n) score matrix as (offsets, indices, scores)."""
    s = np.asarray(scores)
    hit = s >= threshold
    offsets = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
    i, j = np.nonzero(hit)                                # row-major: ascending j within a row
    return offsets, j.astype(np.int64), s[i, j]


def scores64(stored):
    """The float64 score matrix of the self-join of ``stored`` rows: query i is row i normalised again, row j is read as
    stored (an fp16 gallery's rows are not unit length after rounding, so the matrix is not symmetric)."""
    x = np.asarray(stored, dtype=np.float64)
    return (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-6)) @ x.T


def margin64(stored, threshold):
    """The smallest |score - threshold| over all pairs, in float64."""
    return float(np.abs(scores64(stored) - threshold).min())


def model64(stored, threshold, min_samples):
    return model(len(stored), *csr_of(scores64(stored), threshold), min_samples)


def _unit(v):
    return v / np.linalg.norm(v)


def _walk(rng, length, dim, step=0.1, back=8):
    """A random walk on the unit sphere: x[i + 1] = cos(step) x[i] + sin(step) u, u a unit vector orthogonal to the previous
    ``back`` rows - so x[i] . x[i + 1] = cos(step) and x[i] . x[i + 2] = cos(step)^2."""
    x = [_unit(rng.standard_normal(dim))]
    for _ in range(length - 1):
        prev = np.stack(x[-back:], axis=1)                # (dim, <= back)
        u = rng.standard_normal(dim)
        u = u - prev @ np.linalg.lstsq(prev, u, rcond=None)[0]
        x.append(np.cos(step) * x[-1] + np.sin(step) * _unit(u))
    return np.stack(x)


def chains(dim, seed=0):
    """(x (300, dim) fp32, chain (300,)): two walks of 140 and 150 rows (chain 0 and 1) and 10 isolated rows (chain -1),
    shuffled by a fixed permutation so that neighbours lie in different tiles.  With t = 0.9925 (cos 0.1 = 0.9950 above it,
    cos^2 0.1 = 0.9900 below) and min_samples = 3 every inner row of a walk is a core row (itself and two neighbours), the four
    end rows are border rows with one core neighbour each, the isolated rows are noise."""
    rng = np.random.default_rng(100 + seed)
    x = np.concatenate([_walk(rng, 140, dim), _walk(rng, 150, dim), np.stack([_unit(rng.standard_normal(dim)) for _ in range(10)])])
    chain = np.concatenate([np.zeros(140, np.int64), np.ones(150, np.int64), -np.ones(10, np.int64)])
    perm = np.random.default_rng(7).permutation(N_ROWS)
    return x[perm].astype(np.float32), chain[perm]


# rows of the ten special rows of the star fixture: core 1 and its members, core 2 and its members, the tied row, an isolated
# row.  The cores lie in different 128-column tiles, core 1 below core 2.
STAR_ROWS = np.array([40, 3, 150, 271, 200, 130, 9, 299, 128, 64])
STAR_DEGREES = [5, 2, 2, 2, 5, 2, 2, 2, 3, 1]
STAR_LABELS = [0, 0, 0, 0, 1, 1, 1, 1, 0, -1]


def star(dim, seed=0):
    """x (300, dim) fp32: at STAR_ROWS two cores e_0 and e_4, each with three members 0.8 e_c + 0.6 e_m on axes of their own,
    the row (e_0 + e_4) / sqrt(2) - tied between the cores with equal score bits - and one isolated row e_9; every other row is
    a random unit vector on the remaining axes (isolated: no pair of them, and none with a special row, comes near t = 0.7)."""
    assert dim >= 40
    rng = np.random.default_rng(200 + seed)
    x = np.zeros((N_ROWS, dim))
    x[:, 10:] = rng.standard_normal((N_ROWS, dim - 10))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    e = np.eye(dim)
    special = [e[0], 0.8 * e[0] + 0.6 * e[1], 0.8 * e[0] + 0.6 * e[2], 0.8 * e[0] + 0.6 * e[3],
               e[4], 0.8 * e[4] + 0.6 * e[5], 0.8 * e[4] + 0.6 * e[6], 0.8 * e[4] + 0.6 * e[7],
               (e[0] + e[4]) / np.sqrt(2.0), e[9]]
    x[STAR_ROWS] = np.stack(special)
    return x.astype(np.float32)
