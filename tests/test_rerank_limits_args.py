"""The re-ranking limit cases without a GPU (tests/rerank_cases.py, the inputs of test_rerank_limits_gpu.py): the premises of
the cases (the 193-entry set, the restated constants, every row length on its side of its limit, the scan's rows per thread),
the reference's skip rules on examples small enough to check by eye, the margin a plain float32 evaluation leaves of the
tolerance, and every modelled bug missing its case by at least ten times the tolerance or structurally."""
import os
import re

import numpy as np
import pytest

import rerank_cases as C
import rerank_ref as rr
from helpers import ROOT, SCORE_TOL

TOL = C.TOL


def test_restated_constants_are_the_kernels():
    assert TOL == SCORE_TOL == 1e-5
    src = open(os.path.join(ROOT, "imageretrievalresearch_amd", "csrc", "rerank.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    assert int(re.search(r"#define MI355_KR_MAX_K1 (\d+)", hdr).group(1)) == C.MAX_K1 == C.K1
    assert int(re.search(r"constexpr int KR_SCORE_LDS = (\d+);", src).group(1)) == C.KR_SCORE_LDS == 4096
    assert int(re.search(r"constexpr int KR_MAX_DIM = (\d+);", src).group(1)) == C.KR_MAX_DIM == 8192
    assert "KR_MAX_ROW = (KR_MAX_K1 + 1) * ((KR_MAX_K1 + 1) / 2 + 1)" in src and C.MAX_ROW == 561
    scan = src[src.index("void k_kr_scan"):src.index("struct WeightArgs")]
    assert f"__launch_bounds__({C.SCAN_THREADS}) void k_kr_scan" in src
    assert f"(R + {C.SCAN_THREADS - 1}) / {C.SCAN_THREADS}" in scan and f"part[{C.SCAN_THREADS}]" in scan
    sets = src[src.index("void k_kr_sets"):src.index("void k_kr_scan")]
    weights = src[src.index("void k_kr_weights"):src.index("struct LocalArgs")]
    score = src[src.index("void k_kr_score"):src.index("static bool kr_aligned")]
    assert f"for (int i = lane; i < n; i += {C.WAVE})" in sets and "__launch_bounds__(64) void k_kr_sets" in src
    assert f"for (int i = lane; i < n; i += {C.WAVE}) s += out[i]" in weights
    assert f"for (int i = tid; i < n; i += {C.THREADS}) out[i] = out[i] / tot" in weights
    assert f"for (int i = lane; i < ng; i += {C.WAVE})" in score and "if (nq <= KR_SCORE_LDS)" in score
    assert "hipLaunchKernelGGL(k_kr_scan, dim3(1), dim3(1024)" in src


def test_scan_rows_per_thread_and_a_dropped_or_doubled_run():
    assert [C.scan_chunk(R) for R in (1, 1024, 1025, 2048, 2049, 2500, 100_000)] == [1, 1, 2, 2, 3, 3, 98]
    for R in (1024, 1025, 2500):
        counts = np.random.default_rng(R).integers(1, 9, R)
        want = np.concatenate([[0], np.cumsum(counts)])
        assert np.array_equal(C.scan_model(counts), want), R
        for bug in ("dropped", "doubled"):
            got = C.scan_model(counts, bug)
            if C.scan_chunk(R) == 1:                                 # one row per thread: a run has no second row to lose
                assert np.array_equal(got, want), (R, bug)
            else:
                assert not np.array_equal(got, want) and got[-1] != want[-1], (R, bug)


def test_the_hand_made_graph_reaches_193_entries():
    g = C.graph193()
    assert g.shape == (193, 32) and g.min() == 0 and g.max() == 192
    assert all(len(set(row)) == 32 and r not in row for r, row in enumerate(g))
    h = 16
    for c in range(1, 33):
        rh = rr.recip_h(g, c, h)
        assert len(rh) == 17 and len(rh & set(range(33))) == 12 and g[c, 16] == 0
    assert rr.base_set(0, g[0], g) == set(range(33)) and rr.recip_h(g, 0, h) == {0}
    S = rr.sets(g, g)
    lens = [len(s) for s in S]
    assert lens[0] == 193 and S[0] == list(range(193))
    assert sum(n > C.WAVE for n in lens) == 20 and sum(n > 2 * C.WAVE for n in lens) == 1 and max(lens) <= C.MAX_ROW == 561
    assert all(S[r] == sorted({r, 1 + (r - 33) // 5}) for r in range(33, 193))          # a leaf and its owner
    # as query rows every listed row is a member (at equality too), and one step below tau it is not
    lists, vals, tau = C.query193()
    Q = rr.sets(lists, g, vals, tau)
    assert Q[0] == list(range(1, 193)) and len(Q[0]) == 192 > 2 * C.WAVE
    assert rr.sets(*C.query193(equal=5)[:1], g, *C.query193(equal=5)[1:]) == Q
    below = rr.sets(lists, g, vals, C.query193(below=5)[2])
    assert 5 not in rr.base_set(0, lists[0], g, vals[0], C.query193(below=5)[2]) and below != Q
    # a fill that drops its second trip leaves every entry past the first 64 unwritten
    for s in (S[0], S[1], S[40]):
        unsorted = list(np.random.default_rng(1).permutation(s))
        assert C.fill_model(unsorted).tolist() == s
        dropped = C.fill_model(unsorted, "dropped")
        assert (dropped == C.SENTINEL).sum() == max(len(s) - C.WAVE, 0)


def test_reference_skips_bad_ids_by_hand():
    # four rows, k1 = 2 (h = 1): 0 <-> 1 are mutual first neighbours; row 2 lists a pad and itself; row 3 lists 2 twice
    g = np.array([[1, 4], [0, -1], [-1, 2], [2, 2]])
    assert rr.recip_h(g, 0, 1) == {0, 1} and rr.recip_h(g, 2, 1) == {2} and rr.recip_h(g, 3, 1) == {3}
    assert rr.base_set(0, g[0], g) == {0, 1}                         # 4 = G is no member
    assert rr.base_set(2, g[2], g) == {2}                            # the pad and the row itself add nothing
    assert rr.base_set(3, g[3], g) == {3}                            # 2 does not list 3, however often 3 lists it
    assert rr.sets(g, g) == [[0, 1], [0, 1], [2], [3]]
    # R_h with a pad and a repeat inside the first h = 2: c = 0 lists 1 twice, 1 lists 0 -> {0, 1}, counted once
    g2 = np.array([[1, 1, 2], [0, 5, 2], [0, 1, -1]])
    assert rr.recip_h(g2, 0, 2) == {0, 1} and rr.recip_h(g2, 1, 2) == {0, 1} and rr.recip_h(g2, 2, 2) == {2}
    # query rows: a bad id is no member; of a repeated id the first occurrence decides
    tau = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    lists = np.array([[-1, 4], [5, 3], [2, 2], [2, 2]])
    vals = np.array([[0.9, 0.9], [0.9, 0.5], [0.4, 0.6], [0.6, 0.4]], np.float32)
    assert [rr.base_set(r, lists[r], g, vals[r], tau) for r in range(4)] == [set(), {3}, set(), {2}]
    assert rr.sets(lists, g, vals, tau) == [[], [3], [], [2]]
    # weights: a bad column weighs 0 and stays out of the sum
    gal = np.eye(3)
    w = rr.weights(np.eye(3)[:1], gal, [[-1, 0, 1, 3]])[0]
    e0, e1 = 1.0, np.exp(-1.0)
    assert w[-1] == 0.0 and w[3] == 0.0 and w[0] == pytest.approx(e0 / (e0 + e1), abs=1e-15) and sum(w.values()) == pytest.approx(1)
    # local_qe: a bad source is absent, the divisor stays k2; a repeated source is added per occurrence
    V = [{0: 0.5, 1: 0.5}, {1: 1.0}]
    own = [{0: 1.0}]
    assert rr.local_qe(own, V, np.array([[-1, 2, 1]]), 4) == [{0: 0.25, 1: 0.25}]
    assert rr.local_qe(own, V, np.array([[1, 1, 0]]), 3) == [{0: 1 / 3, 1: 2 / 3}]
    assert rr.local_qe(own, V, np.array([[3, -1, 2]]), 4) == [{0: 0.25}]
    # scores: a slot outside [0, G) is -inf
    s = rr.scores([{0: 1.0}], V, np.array([[0.5, 0.5, 0.5, 0.5]]), np.array([[-1, 0, 2, 3]]), 0.3)
    m = 0.5
    assert np.isneginf(s[0, [0, 2, 3]]).all() and s[0, 1] == pytest.approx(1 - (0.7 * (1 - m / (2 - m)) + 0.3 * 0.5), abs=1e-15)
    # broken offsets read as empty rows
    o, c, v, nnz = C.broken_csr()
    rows = C.read_csr_guarded(o, c, v, nnz)
    assert [sorted(r) for r in rows] == [[10 * i + t for t in range(4)] for i in range(6)]
    got = {k: [sorted(r) for r in C.read_csr_guarded(*C.broken_csr(k))] for k in C.BROKEN}
    assert got["hi_below_lo"][2] == [] and got["hi_below_lo"][3] == [13, 20, 21, 22, 23, 30, 31, 32, 33]
    assert got["hi_past_nnz"][5] == [] and got["hi_past_nnz"][:5] == [sorted(r) for r in rows[:5]]
    assert got["lo_negative"][0] == [] and got["lo_negative"][1:] == [sorted(r) for r in rows[1:]]


def test_bad_id_variants_and_a_pad_read_as_the_last_row():
    g, gb = C.graph193(), C.graph193_bad()
    G = C.G193
    assert sorted(set(gb[(gb < 0) | (gb >= G)])) == [-1, G, G + 1]
    Sb = rr.sets(gb, gb)
    assert len(Sb[0]) == 192 and 42 not in Sb[0] and Sb[42] == [42] and Sb[40] == [2, 40] and len(Sb[0]) > 2 * C.WAVE
    # the repeated id of row 30 counted twice would fail 3 |common| > 2 |R_h|
    r = C.BAD_DUP_ROW
    first = [int(j) for j in gb[r][:16]]
    assert len(first) - len(set(first)) == 1
    rh = rr.recip_h(gb, r, 16)
    common = len(rh & set(range(33)))
    assert len(rh) == 16 and 3 * common > 2 * len(rh) and not 3 * common > 2 * (len(rh) + 1)
    # a pad treated as row G - 1 (NumPy's own reading of -1) changes the sets
    wrapped = np.where((gb < 0) | (gb >= G), G - 1, gb)
    assert rr.sets(wrapped, wrapped) != Sb
    lists, vals, tau = C.query193_bad()
    Qb = rr.sets(lists, gb, vals, tau)
    j = int(lists[1, 4])
    assert j == lists[1, 9] and vals[1, 4] < tau[j] <= vals[1, 9] and j not in Qb[1]
    assert Qb[2] == [] and 7 in Qb[7] and all(0 <= c < G for s in Qb for c in s)
    assert rr.sets(np.where((lists < 0) | (lists >= G), G - 1, lists), gb, vals, tau)[0] != Qb[0]
    # the merge sources
    lq, own, gal = C.qe_case()
    lb, _, _ = C.qe_case(bad=True)
    assert lq.shape == (C.L_R, 32) and C.K2 == 33 and list(lq[1]).count(7) == 2 and own[2] == {} and gal[33] == {}
    assert sorted(set(lb[(lb < 0) | (lb >= C.L_G)])) == [-1, C.L_G, C.L_G + 1] and (lb[3] == -1).all()
    good, bad = rr.local_qe(own, gal, lq, C.K2), rr.local_qe(own, gal, lb, C.K2)
    assert bad[3] == {c: x / C.K2 for c, x in own[3].items()} and bad[2] == good[2] and bad[0] != good[0]
    wrap = rr.local_qe(own, gal, np.where((lb < 0) | (lb >= C.L_G), C.L_G - 1, lb), C.K2)
    worst = max(abs(wrap[3].get(c, 0.0) - bad[3].get(c, 0.0)) for c in set(wrap[3]) | set(bad[3]))
    assert set(wrap[3]) != set(bad[3]) and worst >= 10 * TOL


def _weights_operands(D, half):
    gal = C.unit_rows(C.W_G, D, 1)
    rows = C.unit_rows(len(C.W_LENGTHS), D, 2)
    if half:
        gal, rows = gal.astype(np.float16).astype(np.float32), rows.astype(np.float16).astype(np.float32)
    return rows, gal


@pytest.mark.parametrize("D", C.W_DIMS)
def test_weight_rows_margin_and_dropped_trips(D):
    offsets, cols = C.weight_pattern()
    lens = np.diff(offsets).tolist()
    assert lens == list(C.W_LENGTHS) and {0, 1, C.WAVE, C.WAVE + 1, C.THREADS, C.THREADS + 1} <= set(lens)
    assert max(lens) > 2 * C.THREADS and C.W_G >= 600 and cols.max() < C.W_G and D <= C.KR_MAX_DIM
    assert all((np.diff(cols[offsets[r]:offsets[r + 1]]) > 0).all() for r in range(len(lens)))
    for half in (False, True):
        rows, gal = _weights_operands(D, half)
        sets = [cols[offsets[r]:offsets[r + 1]] for r in range(len(lens))]
        want = rr.to_csr(rr.weights(rows.astype(np.float64), gal.astype(np.float64), sets), with_vals=True)[2]
        got = C.weights_model(rows, gal, offsets, cols).astype(np.float64)
        err = np.abs(got - want).max()
        print(f"weights D={D} half={half}: max |float32 - f64| {err:.3e} = {err / TOL:.4f} TOL")
        assert err <= TOL / 10, (D, half, err)
        for bug, hit in (("sum_trip", [n > C.WAVE for n in lens]), ("div_trip", [n > C.THREADS for n in lens])):
            moved = np.abs(C.weights_model(rows, gal, offsets, cols, bug).astype(np.float64) - want)
            per_row = [moved[offsets[r]:offsets[r + 1]].max() if lens[r] else 0.0 for r in range(len(lens))]
            assert all((m >= 10 * TOL) == h for m, h in zip(per_row, hit)), (D, half, bug, per_row)
        ob, cb = C.weight_pattern(bad=True)
        assert np.array_equal(ob, offsets) and sorted(set(cb[(cb < 0) | (cb >= C.W_G)])) == [-1, C.W_G, C.W_G + 1]
        setsb = [cb[ob[r]:ob[r + 1]] for r in range(len(lens))]
        wantb = rr.to_csr(rr.weights(rows.astype(np.float64), gal.astype(np.float64), setsb), with_vals=True)[2]
        assert np.abs(C.weights_model(rows, gal, ob, cb).astype(np.float64) - wantb).max() <= TOL / 10
        assert np.abs(C.weights_model(rows, gal, ob, cb, "pad_is_last").astype(np.float64) - wantb).max() >= 10 * TOL


def test_score_rows_margin_and_every_modelled_bug():
    qrows, gal = C.score_case()
    nq = [len(r) for r in qrows]
    assert nq == [C.KR_SCORE_LDS, C.KR_SCORE_LDS + 1, 6000] and C.S_G >= 6000
    assert set(qrows[1]) - set(qrows[0]) == {C.S_EXTRA} and all(qrows[0][c] == qrows[1][c] for c in qrows[0])
    assert sorted(qrows[1]).index(C.S_EXTRA) < C.KR_SCORE_LDS - 1 and not any(C.S_EXTRA in g for g in gal)
    assert [len(gal[C.S_ROWS[n]]) for n in (1, 64, 65, 300)] == [1, C.WAVE, C.WAVE + 1, 300] and gal[C.S_EMPTY] == {}
    for row in qrows[1:] + [gal[g] for g in C.S_ROWS.values()]:
        assert abs(sum(row.values()) - 1) < 1e-12 and (len(row) == 1 or max(row.values()) > 5 * min(row.values()))
    assert 1 - sum(qrows[0].values()) == pytest.approx(qrows[1][C.S_EXTRA]) and all(max(r) < C.S_G for r in qrows)
    slots = [C.S_ROWS[n] for n in (1, 64, 65, 300)]
    sv = np.full((3, 4), 0.5, np.float32)
    si = np.tile(np.array(slots, np.int64), (3, 1))
    q32 = [{c: float(np.float32(v)) for c, v in r.items()} for r in qrows]          # the operands as the kernel holds them
    g32 = [{c: float(np.float32(v)) for c, v in r.items()} for r in gal]
    want = rr.scores(q32, g32, sv, si, C.S_LAM)

    def model(bug=None):
        return np.array([[C.score_model(q32[q], g32[g], 0.5, C.S_LAM, bug) for g in slots] for q in range(3)], np.float64)

    err = np.abs(model() - want).max()
    print(f"score: max |float32 - f64| {err:.3e} = {err / TOL:.4f} TOL")
    assert err <= TOL / 10
    # the 4096- and the 4097-entry rows take the same sums
    assert np.array_equal(model()[0], model()[1]) and np.array_equal(want[0], want[1])
    moved = {bug: np.abs(model(bug) - want) for bug in ("cut_4096", "lane_trip", "search_lo", "search_hi")}
    assert moved["cut_4096"][0].max() == 0 or moved["cut_4096"][0].max() <= TOL / 10    # 4096 entries: nothing to cut
    assert (moved["cut_4096"][1:].max(1) >= 10 * TOL).all()                              # the rows read where they lie
    assert (moved["lane_trip"][:, 2:].max(1) >= 10 * TOL).all() and moved["lane_trip"][:, :2].max() <= TOL / 10
    assert (moved["search_lo"].max(1) >= 10 * TOL).all() and (moved["search_hi"].max(1) >= 10 * TOL).all()
    for K in (1, 5, 100):
        vals, idx = C.shortlist(K)
        assert vals.shape == idx.shape == (3, K) and np.array_equal(idx[0], idx[1]) and np.array_equal(vals[0], vals[1])
        if K > 1:
            assert {-1, C.S_G, *slots} <= set(idx.reshape(-1).tolist())
        s = rr.scores(q32, g32, vals, idx, C.S_LAM)
        assert np.array_equal(np.isneginf(s), (idx < 0) | (idx >= C.S_G)) and np.array_equal(s[0], s[1])
    # a pad read as row G - 1 (the 300-entry row) gets a finite score
    vals, idx = C.shortlist(5)
    wrapped = rr.scores(q32, g32, vals, np.where((idx < 0) | (idx >= C.S_G), C.S_G - 1, idx), C.S_LAM)
    assert np.isfinite(wrapped).all()


def test_local_expansion_margin_at_33_sources():
    lists, own, gal = C.qe_case()
    g32 = [{c: float(np.float32(v)) for c, v in r.items()} for r in gal]
    o32 = [{c: float(np.float32(v)) for c, v in r.items()} for r in own]
    for bad in (False, True):
        lq = C.qe_case(bad)[0]
        want = rr.local_qe(o32, g32, lq, C.K2)
        for r in range(C.L_R):
            got = C.local_qe_model(o32[r], g32, lq[r], C.K2)
            assert sorted(got) == sorted(want[r])
            err = max((abs(float(got[c]) - want[r][c]) for c in got), default=0.0)
            assert err <= TOL / 10, (bad, r, err)
    V2 = rr.local_qe(o32, g32, lists, C.K2)
    assert max(len(v) for v in V2) > 2 * C.WAVE
    for r in range(C.L_R):                                          # every source sums to 1, an empty one to 0
        full = bool(own[r]) + sum(bool(gal[int(j)]) for j in lists[r])
        assert sum(V2[r].values()) == pytest.approx(full / C.K2, abs=1e-6), r
    assert not own[2] and 33 in lists[2]                             # row 2 has an empty own row and an empty source


def test_margin_over_the_193_entry_set():
    """The values the GPU test takes over the hand-made graph: weights at D = 70, then the 33-source merge."""
    g = C.graph193()
    S = rr.sets(g, g)
    x = C.unit_rows(C.G193, 70, 5)
    offsets, cols = rr.to_csr(S)
    V = rr.weights(x.astype(np.float64), x.astype(np.float64), S)
    got = C.weights_model(x, x, offsets, cols).astype(np.float64)
    err = np.abs(got - rr.to_csr(V, with_vals=True)[2]).max()
    assert err <= TOL / 10, err
    V32 = rr.from_csr(offsets, cols, got.astype(np.float32))
    want = rr.local_qe(V32, V32, g, C.K2)
    for r in (0, 1, 40):
        row = C.local_qe_model(V32[r], V32, g[r], C.K2)
        assert sorted(row) == sorted(want[r]) and max(abs(float(row[c]) - want[r][c]) for c in row) <= TOL / 10, r
    assert len(want[0]) == 193
