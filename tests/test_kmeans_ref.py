"""The float64 k-means / clustering-score reference against hand-computed values, and the certificate of the planted inputs
the GPU tests cluster (tests/test_kmeans_gpu.py)."""
import math

import numpy as np
import pytest

import kmeans_ref as ref


def test_identical_labelings_score_one():
    a = np.array([5, 5, -2, 9, 9, 9, -2])
    m = ref.metrics(a, a)
    assert m["nmi"] == pytest.approx(1.0, abs=1e-15) and m["purity"] == 1.0 and m["f1"] == 1.0
    assert m["n_clusters"] == m["n_classes"] == 3
    one = ref.metrics(np.zeros(4, np.int64), np.zeros(4, np.int64))          # both entropies 0
    assert one["nmi"] == 1.0 and one["f1"] == 1.0


def test_hand_computed_table():
    t = np.array([[3, 1], [0, 4]])
    m = ref.metrics_from_table(t)
    # a = (4, 4), b = (3, 5), N = 8
    info = 3 / 8 * math.log(8 * 3 / (4 * 3)) + 1 / 8 * math.log(8 * 1 / (4 * 5)) + 4 / 8 * math.log(8 * 4 / (4 * 5))
    ha = math.log(2)
    hb = -(3 / 8 * math.log(3 / 8) + 5 / 8 * math.log(5 / 8))
    assert m["info"] == pytest.approx(info, abs=1e-15)
    assert m["nmi"] == pytest.approx(2 * info / (ha + hb), abs=1e-15)
    assert m["purity"] == 7 / 8
    # TP = C(3,2) + C(4,2) = 9; sum C(a,2) = 12; sum C(b,2) = 3 + 10 = 13
    assert m["precision"] == 9 / 12 and m["recall"] == 9 / 13
    assert m["f1"] == pytest.approx(2 * (9 / 12) * (9 / 13) / (9 / 12 + 9 / 13), abs=1e-15)


def test_independent_labelings_carry_no_information():
    t = np.outer([2, 3, 5], [1, 4])                      # a product table
    m = ref.metrics_from_table(t)
    assert abs(m["info"]) < 1e-15 and abs(m["nmi"]) < 1e-15


def test_zero_over_zero_counts_as_one():
    m = ref.metrics(np.arange(4), np.zeros(4, np.int64))     # singletons: no pair shares a cluster
    assert m["precision"] == 1.0 and m["recall"] == 0.0 and m["f1"] == 0.0


def test_label_permutation_changes_nothing():
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 6, 500), rng.integers(0, 4, 500)
    m0 = ref.metrics(a, b)
    perm = rng.permutation(6)
    m1 = ref.metrics(perm[a] * 7 - 20, b)
    for k in ("nmi", "purity", "f1", "precision", "recall"):
        assert m1[k] == pytest.approx(m0[k], abs=1e-12), k


def test_contingency_makes_labels_dense_by_sorted_value():
    t, av, bv = ref.contingency(np.array([10, -3, 10, 7]), np.array([2, 2, 0, 2]))
    assert av.tolist() == [-3, 7, 10] and bv.tolist() == [0, 2]
    assert t.tolist() == [[0, 1], [0, 1], [1, 1]]


def test_assign_ties_go_to_the_lower_index_and_update_keeps_empty_clusters():
    x = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 0.0]])
    c = np.array([[0.0, 1.0], [1.0, 0.0], [2.0, 0.0], [-1.0, 0.0]])
    a, s, gap = ref.assign(x, c)
    assert a.tolist() == [1, 0, 1] and np.allclose(s, 1.0) and gap.tolist() == [0.0, 1.0, 0.0]
    out, counts, kept = ref.update(ref.normalise(x), a, 4, c)
    assert counts.tolist() == [1, 2, 0, 0] and kept.tolist() == [False, False, True, True]
    assert out.tolist() == [[0.0, 1.0], [1.0, 0.0], [2.0, 0.0], [-1.0, 0.0]]


@pytest.mark.parametrize("cfg", ref.PLANTED, ids=lambda c: "seed%d-%dx%d-k%d" % c[:4])
def test_planted_inputs_are_certified(cfg):
    """The reference recovers the planted labels exactly and no row ever comes within 1e-4 of a boundary: an fp32
    implementation with 1e-5 scores must make the same assignments in every pass."""
    seed, N, D, K, noise = cfg
    x, lab, init = ref.planted(seed, N, D, K, noise)
    r = ref.kmeans(x, init)
    assert r["converged"] and r["min_gap"] >= 1e-4, r["min_gap"]
    assert r["iterations"] == (2 if D == 70 else 3)
    m = ref.metrics(r["assignments"], lab)
    assert m["nmi"] == pytest.approx(1.0, abs=1e-12) and m["purity"] == 1.0 and m["f1"] == 1.0
    assert (r["assignments"] == lab).all()                 # init row k is planted in cluster k
