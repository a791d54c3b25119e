"""NumPy model of the binary (sign-bit) gallery's numerical contract (include/mi355_retrieval.h), bit for bit: the encoder, the
Hamming distances, the score of a (query, row) pair and the top-k order with a mask.  The contract is integer arithmetic and
one float32 division, so the model has no tolerance anywhere.  Also the planted mixture on which the two recall conditions of
the format are stated (tests/test_binary_ref.py, tests/test_binary_gpu.py)."""
import numpy as np

F32 = np.float32
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def words(dim):
    return (dim + 31) // 32


def encode(n, center=None):
    """codes uint32 [R][ceil(dim / 32)] of the normalised float32 rows n [R][dim]: bit j % 32 of word j / 32 is 1 iff
    n[j] >= center[j] (center None: zeros); a NaN on either side gives 0, pad bits are 0."""
    n = np.ascontiguousarray(n, dtype=F32)
    R, dim = n.shape
    c = np.zeros(dim, F32) if center is None else np.ascontiguousarray(center, dtype=F32)
    with np.errstate(invalid="ignore"):
        bits = n >= c[None, :]                                        # False for a NaN on either side
    W = words(dim)
    padded = np.zeros((R, W * 32), np.uint64)
    padded[:, :dim] = bits
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))[None, None, :]
    return (padded.reshape(R, W, 32) * weights).sum(axis=2).astype(np.uint32)


def has_nan(n):
    """bool [R]: the rows of n with a NaN element (such a QUERY scores NaN everywhere)."""
    return np.isnan(np.asarray(n, dtype=F32)).any(axis=1)


def popcount(x):
    """int64 popcount of every uint32 element."""
    b = np.ascontiguousarray(x, dtype=np.uint32).view(np.uint8).reshape(x.shape + (4,))
    return _POP8[b].sum(axis=-1)


def distances(qcodes, gcodes, qnan=None):
    """int32 [Q][G]: the popcount of the xor of the two code rows; -1 in the rows of the queries flagged in qnan."""
    d = np.empty((qcodes.shape[0], gcodes.shape[0]), np.int32)
    for i in range(qcodes.shape[0]):
        d[i] = popcount(qcodes[i][None, :] ^ gcodes).sum(axis=1)
    if qnan is not None:
        d[np.asarray(qnan, bool)] = -1
    return d


def scores(dist, dim):
    """float32 [Q][G]: float32(dim - 2 h) / float32(dim), one division; NaN where the distance is -1 (a NaN query)."""
    h = np.asarray(dist, np.int64)
    s = (dim - 2 * h).astype(F32) / F32(dim)
    return np.where(h < 0, F32(np.nan), s).astype(F32)


def select(s, k, mask=None):
    """(values float32 [Q][k], indices int64 [Q][k]): a stable sort on (NaN first, -score, row); with a boolean mask [Q][G] of
    eligible rows an ineligible row never appears and the slots past the eligible rows are (-inf, -1)."""
    s = np.asarray(s, dtype=F32)
    key = np.where(np.isnan(s), np.inf, s.astype(np.float64))
    elig = np.ones(s.shape, bool) if mask is None else np.asarray(mask, bool)
    key = np.where(elig, key, -np.inf)
    cols = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    order = np.lexsort((cols, ~elig, -key), axis=1)[:, :k]
    vals = np.take_along_axis(s, order, axis=1).astype(F32)
    pad = np.arange(k)[None, :] >= elig.sum(axis=1)[:, None]
    return np.where(pad, F32(-np.inf), vals).astype(F32), np.where(pad, -1, order.astype(np.int64))


def normalize(x):
    """float32 unit rows, normalised in float64 and rounded once (a host-side input maker, not the library's bits)."""
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def mean_center(n):
    """The float32 rounding of the float64 column mean of the float32 rows n."""
    n = np.asarray(n, F32)
    return (n.astype(np.float64).sum(axis=0) / float(n.shape[0])).astype(F32)


def planted_mixture(seed, D=256, centres=64, noise=1.0, rows=4096, queries=64):
    """(x [rows][D], q [queries][D]) float64: N(0, 1) centres, every row and query a centre plus noise * N(0, 1)."""
    r = np.random.default_rng(seed)
    c = r.standard_normal((centres, D))
    x = c[r.integers(0, centres, rows)] + noise * r.standard_normal((rows, D))
    q = c[r.integers(0, centres, queries)] + noise * r.standard_normal((queries, D))
    return x, q


def pooled(x):
    """The mixture as a pooled activation: clipped at 0 and shifted by +0.3, so every element is positive."""
    return np.maximum(x, 0.0) + 0.3


def refined_recall(n, qn, gcodes, qcodes, k=10, shortlist=100):
    """Recall@k, against the float64 cosine top-k of the unit rows, of: the `shortlist` best rows by binary score (ties to the
    lower row), rescored exactly and cut to k."""
    dim = n.shape[1]
    cos = qn.astype(np.float64) @ n.astype(np.float64).T
    want = np.argsort(-cos, axis=1, kind="stable")[:, :k]
    _, short = select(scores(distances(qcodes, gcodes), dim), shortlist)
    re = np.take_along_axis(cos, short, axis=1)
    got = np.take_along_axis(short, np.argsort(-re, axis=1, kind="stable")[:, :k], axis=1)
    return float(np.mean([len(set(a) & set(b)) / float(k) for a, b in zip(got.tolist(), want.tolist())]))
