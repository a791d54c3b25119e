"""The NumPy model of residual IVF-PQ (ivfrpq_ref.py) against what it is a model of, without a GPU: coding the offset from the
list centroid loses less than coding the whole row where the lists find the clusters, and a model score is the inner product of
the query with ``centroid + reconstruction`` up to float32 rounding."""
import numpy as np

import ivfrpq_ref as V
import pq_ref as R
from helpers import SCORE_TOL
from imageretrievalresearch_amd.cluster import seeded_rows

N, D, M, NLIST, SEED = 4096, 64, 16, 32, 0
_cache = {}


def _case():
    """Rows around 32 centres, the lists of a 10-step spherical k-means from the project's seeded start, and both 6-step
    codebooks (plain and residual) from the same 256 seeded rows."""
    if not _cache:
        n = R.clustered_rows(N, D, 32, 0.3, SEED)
        c, a = V.kmeans_lists(n, NLIST, 10, seeded_rows(N, NLIST, SEED))
        pick = seeded_rows(N, 256, SEED)
        plain_cb, plain = R.lloyd(n, M, 6, pick)
        cb, resid = V.train(n, a, c, M, 6, pick)
        _cache.update(n=n, c=c, a=a, plain_cb=plain_cb, plain=plain[-1], cb=cb, resid=resid[-1])
    return _cache


def test_residual_codes_lose_less_than_plain_codes():
    # measured: residual / plain quantisation error = 0.450 (0.01407 / 0.03130); recall@10 against the exact order, below:
    # 0.328 -> 0.442.  The bound 0.75 sits halfway between an ad-hoc k-means' 0.47 and no gain at all.
    m = _case()
    codes = V.encode(m["n"], m["a"], m["c"], m["cb"])
    err = V.quantisation_error(m["n"], V.reconstruct(codes, m["a"], m["c"], m["cb"]))
    print(f"quantisation error: plain {m['plain']:.5f}, residual {err:.5f}, ratio {err / m['plain']:.3f}")
    assert abs(err - m["resid"]) < 1e-6                  # the distortion of the residual rows is the error of the rows
    assert err < 0.75 * m["plain"]


def test_recall_of_the_model_does_not_fall():
    m = _case()
    n = m["n"]
    q, g = n[:64], n
    exact = np.argsort(-(q.astype(np.float64) @ g.astype(np.float64).T), axis=1, kind="stable")[:, :10]
    plain = R.topk(R.scores(R.table(q, m["plain_cb"]), R.encode(g, m["plain_cb"])), 10)[1]
    codes = V.encode(g, m["a"], m["c"], m["cb"])
    s = V.scores(V.coarse32(q, m["c"]), q, m["cb"], codes, m["a"])
    resid = V.search(s, 10, m["a"], NLIST, np.tile(np.arange(NLIST), (64, 1)))[1]
    rec = [np.mean([len(set(e) & set(r)) / 10.0 for e, r in zip(exact, got)]) for got in (plain, resid)]
    print(f"recall@10 vs exact: plain {rec[0]:.3f}, residual {rec[1]:.3f}")
    assert rec[1] >= rec[0]


def test_model_score_is_the_inner_product_with_the_reconstruction():
    m = _case()
    q = R.clustered_rows(50, D, 32, 0.3, SEED + 1)
    codes = V.encode(m["n"], m["a"], m["c"], m["cb"])
    s = V.scores(V.coarse32(q, m["c"]), q, m["cb"], codes, m["a"])
    recon64 = m["c"].astype(np.float64)[m["a"]] + R.reconstruct(codes, m["cb"]).astype(np.float64)
    want = q.astype(np.float64) @ recon64.T
    print(f"max |model - float64| = {np.abs(s - want).max():.2e}")
    assert np.abs(s - want).max() < SCORE_TOL


def test_search_is_restricted_to_the_probed_lists_and_pads():
    m = _case()
    q = m["n"][:5]
    codes = V.encode(m["n"], m["a"], m["c"], m["cb"])
    s = V.scores(V.coarse32(q, m["c"]), q, m["cb"], codes, m["a"])
    probes = np.array([[3, 7]] * 5)
    v, i = V.search(s, 10, m["a"], NLIST, probes)
    assert np.isin(m["a"][i[i >= 0]], [3, 7]).all()
    every = V.search(s, 10, m["a"], NLIST, np.tile(np.arange(NLIST)[::-1], (5, 1)))
    assert (every[1] == R.topk(s, 10)[1]).all()          # every list, any order: the exhaustive top-k
    short = np.nonzero(np.bincount(m["a"], minlength=NLIST) < 300)[0][:1]
    v, i = V.search(s, 300, m["a"], NLIST, np.tile(short, (5, 1)))
    assert (i[:, -1] == -1).all() and np.isneginf(v[:, -1]).all()
    lab = np.arange(N) % 3
    v, i = V.search(s, 10, m["a"], NLIST, probes, query_labels=np.zeros(5, np.int64), gallery_labels=lab, label_filter="same",
                    exclude=np.full(5, -1), idx_offset=100)
    assert (lab[i[i >= 0] - 100] == 0).all()
