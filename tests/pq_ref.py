"""NumPy model of the product-quantised gallery's numerical contract (include/mi355_retrieval.h), bit for bit: the encoder, the
query tables, the score of a (query, row) pair, the centroid update and the top-k order with a mask.  Every fp32 operation of
the contract is one float32 NumPy operation here (a product is rounded before it is added: no fma); the update's float64 sums
run over the members one at a time in ascending row order (np.add.at is unbuffered and goes through its indices in order)."""
import numpy as np

from gallery_i8_ref import topk  # noqa: F401  (the selection is the same: descending, NaN first, ties to the lower row, pads)

F32 = np.float32
CENTROIDS = 256


def _sub(n, M):
    n = np.ascontiguousarray(n, dtype=F32)
    return n.reshape(n.shape[0], M, n.shape[1] // M)


def encode(n, cb):
    """codes uint8 [R][M] of the normalised float32 rows n [R][dim] against the codebooks cb [M][256][dsub]."""
    cb = np.ascontiguousarray(cb, dtype=F32)
    M, _, dsub = cb.shape
    x = _sub(n, M)
    codes = np.empty((x.shape[0], M), np.uint8)
    with np.errstate(all="ignore"):
        for m in range(M):
            d = np.zeros((x.shape[0], CENTROIDS), F32)
            for i in range(dsub):
                t = x[:, m, i][:, None] - cb[m, :, i][None, :]
                d = d + t * t
            # the lowest c whose d is strictly below every earlier one; a NaN is never below anything
            codes[:, m] = np.argmin(np.where(np.isnan(d), F32(np.inf), d), axis=1)
    return codes


def table(qn, cb):
    """T float32 [Q][M][256]: acc = acc + qn[m*dsub+i] * cb[m][c][i] for i ascending."""
    cb = np.ascontiguousarray(cb, dtype=F32)
    M, _, dsub = cb.shape
    x = _sub(qn, M)
    T = np.zeros((x.shape[0], M, CENTROIDS), F32)
    with np.errstate(all="ignore"):
        for i in range(dsub):
            T = T + x[:, :, i][:, :, None] * cb[None, :, :, i]
    return T


def scores(T, codes):
    """float32 [Q][G]: a[m % 4] += T[m][code[g][m]] for m ascending, then (a0 + a1) + (a2 + a3)."""
    Q, M, _ = T.shape
    a = np.zeros((4, Q, codes.shape[0]), F32)
    with np.errstate(all="ignore"):
        for m in range(M):
            a[m % 4] = a[m % 4] + T[:, m, :][:, codes[:, m]]
        return (a[0] + a[1]) + (a[2] + a[3])


def update(n, codes, cb):
    """(codebooks float32 [M][256][dsub], counts int64 [M][256]): the float64 mean of every cell's members, added in ascending
    row order, rounded once; an empty cell keeps cb's centroid."""
    cb = np.ascontiguousarray(cb, dtype=F32)
    M, _, dsub = cb.shape
    x = _sub(n, M).astype(np.float64)
    out = cb.copy()
    counts = np.zeros((M, CENTROIDS), np.int64)
    for m in range(M):
        s = np.zeros((CENTROIDS, dsub), np.float64)
        np.add.at(s, codes[:, m], x[:, m, :])
        counts[m] = np.bincount(codes[:, m], minlength=CENTROIDS)
        live = counts[m] > 0
        out[m, live] = (s[live] / counts[m, live, None].astype(np.float64)).astype(F32)
    return out, counts


def reconstruct(codes, cb):
    """float32 [R][dim]: the concatenation of the centroids the codes name."""
    M = cb.shape[0]
    return cb[np.arange(M)[None, :], codes].reshape(codes.shape[0], -1)


def distortion(n, codes, cb):
    """The float64 mean squared distance of the rows to their reconstruction."""
    d = np.asarray(n, np.float64) - reconstruct(codes, np.asarray(cb, F32)).astype(np.float64)
    return float((d * d).sum(axis=1).mean())


def clustered_rows(N, D, centres, noise, seed):
    """N float32 rows around `centres` seeded directions, L2-normalised in float64 and rounded: a trainable input."""
    r = np.random.RandomState(seed)
    c = r.standard_normal((centres, D))
    x = c[r.randint(0, centres, N)] + noise * r.standard_normal((N, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def lloyd(n, M, iters, pick):
    """The codebooks after each of `iters` encode + update steps from the rows `pick` (256 indices), and the distortion after
    every step (index 0: of the start)."""
    n = np.ascontiguousarray(n, dtype=F32)
    dsub = n.shape[1] // M
    cb = np.ascontiguousarray(n[pick].reshape(CENTROIDS, M, dsub).transpose(1, 0, 2))
    dist = []
    for _ in range(iters):
        codes = encode(n, cb)
        dist.append(distortion(n, codes, cb))
        cb, _ = update(n, codes, cb)
    dist.append(distortion(n, encode(n, cb), cb))
    return cb, dist
