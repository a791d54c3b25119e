"""NumPy model of the residual IVF-PQ contract (include/mi355_retrieval.h), on top of pq_ref.py: the codes describe
``rn - centroids[list]`` (one float32 subtraction per element), training is pq_ref.lloyd on those rows, and the score of a
(query, row) pair is ``float32(coarse[q][list of the row] + the PQ score of its code row)``.  The coarse term is an input here:
the library takes it from its one-wave-per-pair dot (whose bits the GPU tests read from ``index.coarse``); ``coarse32`` is a
plain float32 stand-in for the CPU tests.  Which rows a query sees, eligibility and the top-k are ivf_ref.py's and pq_ref.topk."""
import numpy as np

import ivf_ref as I
import kmeans_ref as K
import pq_ref as R

F32 = np.float32


def residuals(n, assign, centroids):
    """float32 [N][D]: n[r] - centroids[assign[r]], each element one float32 subtraction."""
    n, c = np.ascontiguousarray(n, dtype=F32), np.ascontiguousarray(centroids, dtype=F32)
    return n - c[np.asarray(assign, np.int64)]


def train(n, assign, centroids, M, iters, pick):
    """(codebooks, distortions) of pq_ref.lloyd over the residual rows from the 256 rows ``pick`` of them."""
    return R.lloyd(residuals(n, assign, centroids), M, iters, pick)


def encode(n, assign, centroids, cb):
    return R.encode(residuals(n, assign, centroids), cb)


def reconstruct(codes, assign, centroids, cb):
    """float32 [N][D]: centroids[assign] + the centroids the residual codes name (one float32 addition per element)."""
    return np.ascontiguousarray(centroids, dtype=F32)[np.asarray(assign, np.int64)] + R.reconstruct(codes, np.asarray(cb, F32))


def coarse32(qn, centroids):
    """float32 [Q][nlist]: a float32 matrix product, for the CPU tests (not the library's summation order)."""
    return np.ascontiguousarray(qn, dtype=F32) @ np.ascontiguousarray(centroids, dtype=F32).T


def scores(coarse, qn, cb, codes, assign):
    """float32 [Q][G]: coarse[q][assign[g]] + pq_ref.scores(table(qn, cb), codes)[q][g], one float32 addition.  ``coarse`` is
    float32 [Q][nlist]."""
    s = R.scores(R.table(qn, cb), codes)
    with np.errstate(all="ignore"):
        return (np.asarray(coarse, F32)[:, np.asarray(assign, np.int64)] + s).astype(F32)


def probed_mask(assign, nlist, probes):
    """bool [Q][G]: the rows of every query's probed lists."""
    offsets, order = I.lists_of(assign, nlist)
    mask = np.zeros((len(probes), len(assign)), bool)
    for qi, p in enumerate(probes):
        mask[qi, I.probed_rows(offsets, order, p)] = True
    return mask


def search(s, k, assign, nlist, probes, **filt):
    """(values float32 [Q][k], indices [Q][k]) of the model's scores ``s`` over the probed, eligible rows: pq_ref.topk
    (descending, NaN first, ties to the lower gallery row, pads (-inf, -1)).  ``filt``: the arguments of ivf_ref.eligible;
    indices come back with ``idx_offset`` added."""
    Q, G = s.shape
    mask = probed_mask(assign, nlist, probes)
    if filt:
        mask &= I.eligible(G, Q, **filt)
    v, i = R.topk(s, k, mask)
    return v, np.where(i >= 0, i + filt.get("idx_offset", 0), -1)


def quantisation_error(n, recon):
    """float64: the mean squared distance of the rows to their reconstruction."""
    d = np.asarray(n, np.float64) - np.asarray(recon, np.float64)
    return float((d * d).sum(axis=1).mean())


def kmeans_lists(n, nlist, iters, pick):
    """(centroids float32 [nlist][D], assign [N]): kmeans_ref's spherical k-means from the rows ``pick``; the assignments are
    those of the rounded centroids, as an index would make them."""
    c = K.kmeans(n, np.asarray(n, np.float64)[pick], iters)["centroids"].astype(F32)
    return c, K.assign(n, c)[0]
