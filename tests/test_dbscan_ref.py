"""The NumPy model of DBSCAN (tests/dbscan_ref.py) on hand-written graphs, its fixtures' expected structure in float64, and the
model against sklearn where sklearn is installed.  No GPU."""
import numpy as np
import pytest

import dbscan_ref as ref


def _csr(n, hits):
    """CSR of directed hits {(i, j): score}; every row hits itself with score 1."""
    full = {(i, i): 1.0 for i in range(n)}
    full.update(hits)
    rows = [sorted((j, s) for (i, j), s in full.items() if i == r) for r in range(n)]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.array([j for r in rows for j, _ in r], dtype=np.int64)
    scores = np.array([s for r in rows for _, s in r], dtype=np.float32)
    return offsets, indices, scores


def _sym(pairs):
    return {k: s for (i, j), s in pairs.items() for k in ((i, j), (j, i))}


def test_border_row_between_two_clusters_takes_the_higher_score_then_the_lower_core_row():
    # cores 1 (with 0, 2) and 5 (with 4, 6); row 3 hits both cores
    base = {(1, 0): .9, (1, 2): .9, (5, 4): .9, (5, 6): .9}

    def labels(s13, s53):
        hits = _sym({**base, (1, 3): s13, (5, 3): s53})
        return ref.model(7, *_csr(7, hits), 4)

    m = labels(0.8, 0.8)                                  # a tie: the lower core row
    assert m["core"].tolist() == [False, True, False, False, False, True, False]
    assert m["degree"].tolist() == [2, 4, 2, 3, 2, 4, 2]
    assert m["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1] and m["roots"].tolist() == [1, 5] and m["counts"].tolist() == [4, 3]
    assert labels(0.8, 0.81)["labels"].tolist() == [0, 0, 0, 1, 1, 1, 1]        # the higher score wins over the lower row
    assert labels(0.81, 0.8)["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert labels(-0.0, 0.0)["labels"].tolist() == [0, 0, 0, 0, 1, 1, 1]        # -0 ties with +0


def test_a_hit_in_one_direction_links_cores_and_offers_a_border_row():
    # 0 - 1 symmetric; hit(2, 1) only (row 1 does not hit row 2); hit(0, 3) only
    hits = {(0, 1): .9, (1, 0): .9, (2, 1): .85, (0, 3): .7}
    m = ref.model(4, *_csr(4, hits), 2)
    assert m["degree"].tolist() == [3, 2, 2, 1] and m["core"].tolist() == [True, True, True, False]
    assert m["labels"].tolist() == [0, 0, 0, 0] and m["roots"].tolist() == [0]   # 2 joins through its own hit; 3 is border
    m = ref.model(4, *_csr(4, hits), 3)                   # only row 0 is core: 1 and 3 are its border rows, 2 reaches no core
    assert m["core"].tolist() == [True, False, False, False] and m["labels"].tolist() == [0, 0, -1, 0]
    # the border candidate of a one-directional hit carries that direction's score: row 1 between cores 0 (hit(0, 1) = .9)
    # and 2 (hit(2, 1) = .95, and no hit(1, 2))
    hits = {(0, 1): .9, (1, 0): .9, (2, 1): .95, (0, 3): .9, (3, 0): .9, (2, 4): .9, (4, 2): .9, (0, 5): .9, (2, 5): .9, (2, 6): .9}
    m = ref.model(7, *_csr(7, hits), 4)
    assert m["core"].tolist() == [True, False, True, False, False, False, False]
    assert m["labels"].tolist() == [0, 1, 1, 0, 1, 0, 1]


def test_min_samples_one_is_connected_components():
    hits = _sym({(0, 5): .9, (5, 2): .9, (1, 4): .9}) | {(3, 4): .9}
    m = ref.model(7, *_csr(7, hits), 1)
    assert m["core"].all() and (m["labels"] >= 0).all()
    assert m["labels"].tolist() == [0, 1, 0, 1, 1, 0, 2] and m["roots"].tolist() == [0, 1, 6] and m["counts"].tolist() == [3, 3, 1]
    assert ref.model(7, *_csr(7, hits), 8)["labels"].tolist() == [-1] * 7         # above every degree: all noise
    one = ref.model(1, *_csr(1, {}), 1)
    assert one["labels"].tolist() == [0] and one["roots"].tolist() == [0] and one["degree"].tolist() == [1]


@pytest.mark.parametrize("dim", [70, 96])
def test_fixtures_have_the_structure_the_gpu_tests_expect(dim):
    x, chain = ref.chains(dim)
    assert x.shape == (ref.N_ROWS, dim) and x.dtype == np.float32
    for rows in (x, x.astype(np.float16).astype(np.float32)):
        assert ref.margin64(rows, ref.CHAIN_T) >= 1e-3
        m = ref.model64(rows, ref.CHAIN_T, ref.CHAIN_MIN)
        assert sorted(m["counts"].tolist()) == [140, 150] and int(m["core"].sum()) == 286
        assert int(((m["labels"] >= 0) & ~m["core"]).sum()) == 4 and int((m["labels"] < 0).sum()) == 10
        assert ((m["labels"] < 0) == (chain < 0)).all()
        for c in (0, 1):                                  # a walk is one cluster
            assert len(set(m["labels"][chain == c].tolist())) == 1
        assert len(set(ref.model64(rows, ref.CHAIN_T, 1)["labels"].tolist())) == 12     # components: the walks and 10 single rows
    s = ref.star(dim)
    for rows in (s, s.astype(np.float16).astype(np.float32)):
        assert ref.margin64(rows, ref.STAR_T) >= 1e-3
        m = ref.model64(rows, ref.STAR_T, ref.STAR_MIN)
        assert m["degree"][ref.STAR_ROWS].tolist() == ref.STAR_DEGREES
        assert m["labels"][ref.STAR_ROWS].tolist() == ref.STAR_LABELS
        rest = np.setdiff1d(np.arange(ref.N_ROWS), ref.STAR_ROWS)
        assert (m["degree"][rest] == 1).all() and (m["labels"][rest] == -1).all()
        assert ref.STAR_ROWS[0] // 128 != ref.STAR_ROWS[4] // 128 and ref.STAR_ROWS[0] < ref.STAR_ROWS[4]


def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("dim", [70, 96])
def test_model_agrees_with_sklearn(dim):
    cluster = pytest.importorskip("sklearn.cluster")

    def sk(rows, t, ms):
        s = ref.scores64(rows)
        d = np.clip(1.0 - np.maximum(s, s.T), 0.0, None)  # a hit in either direction is a neighbour
        np.fill_diagonal(d, 0.0)
        est = cluster.DBSCAN(eps=1.0 - t, min_samples=ms, metric="precomputed").fit(d)
        core = np.zeros(len(rows), dtype=bool)
        core[est.core_sample_indices_] = True
        return est.labels_, core

    x, _ = ref.chains(dim)
    labels, core = sk(x, ref.CHAIN_T, ref.CHAIN_MIN)
    m = ref.model64(x, ref.CHAIN_T, ref.CHAIN_MIN)
    assert (m["core"] == core).all() and ((m["labels"] < 0) == (labels < 0)).all()
    assert _same_partition(m["labels"], labels)          # each border row has one core neighbour: no order dependence
    s = ref.star(dim)
    labels, core = sk(s, ref.STAR_T, ref.STAR_MIN)
    m = ref.model64(s, ref.STAR_T, ref.STAR_MIN)
    assert (m["core"] == core).all() and ((m["labels"] < 0) == (labels < 0)).all()
    assert _same_partition(m["labels"][core], labels[core])
