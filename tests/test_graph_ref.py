"""The NumPy model of the graph index (tests/graph_ref.py) against brute force, and ``merged_graph`` of graph.py (torch sorts,
run here on CPU tensors) against the model's loop.  No GPU."""
import numpy as np
import pytest
import torch

import graph_ref as ref
from imageretrievalresearch_amd import MI355Error, graph


def _complete(G):
    return np.stack([[j for j in range(G) if j != r] for r in range(G)]).astype(np.int32)


def test_complete_graph_with_a_wide_beam_is_the_exact_topk():
    rng = np.random.default_rng(0)
    G, Q = 23, 7
    S = rng.standard_normal((Q, G)).astype(np.float32)
    S[2, 5] = np.nan                                                     # NaN ranks first
    S[3, [4, 9]] = 0.25                                                  # a tie: the lower row first
    S[4, 3], S[4, 8] = 0.0, -0.0                                         # -0 equals +0
    seeds = rng.integers(0, G, (Q, 2))
    for k in (1, 3, G):
        v, i, iters, visited = ref.search(S, _complete(G), seeds, k, G + 5, 100)
        for q in range(Q):
            wv, wi = ref.topk_exact(S[q], k)
            assert (i[q] == wi).all() and (v[q].view(np.int32) == wv.view(np.int32)).all(), (k, q)
        assert (visited == G).all() and (iters == G).all()               # every row enters the beam and is expanded once
    assert ref.search(S, _complete(G), seeds, 1, G, 100)[1][2, 0] == 5
    i3 = ref.search(S, _complete(G), seeds, G, G, 100)[1][3].tolist()
    assert i3.index(4) + 1 == i3.index(9)
    i4 = ref.search(S, _complete(G), seeds, G, G, 100)[1][4].tolist()
    assert i4.index(3) + 1 == i4.index(8)


def test_equal_zero_and_nan_scores_in_a_narrow_beam_keep_the_beam_order():
    """The scores of test_graph_gpu's order test - copies r and r + 30 with equal scores, a run of exact zeros of both signs,
    NaNs - walked over a sparse ring with beams narrower than the ties: after every merge the beam is the best ef rows seen in
    the strict order (NaN first, descending, -0 = +0, the lower row), so no two rows ever share a place."""
    G, Q = 60, 4
    rng = np.random.default_rng(5)
    half = rng.standard_normal((Q, G // 2)).astype(np.float32)
    S = np.concatenate([half, half], axis=1)                             # rows r and r + 30 tie, for every r
    S[:, 10:14] = 0.0
    S[:, 40:44] = -0.0                                                   # eight zeros, four of them negative
    S[0, 7] = S[1, [7, 37, 52]] = np.nan                                 # one NaN; three NaNs, one beside its own copy
    S[3] = 0.0                                                           # a query that ties with everything ...
    S[3, 20] = np.nan                                                    # ... but one NaN row
    graph = np.stack([[(r + 1) % G, (r - 1) % G, (r + 30) % G, (r + 7) % G] for r in range(G)]).astype(np.int32)
    seeds = np.array([[0, 31], [59, 7], [12, 42], [45, 2]])
    for ef in (2, 5, 9, G):
        for k in (1, min(ef, 9), ef):
            v, i, iters, visited = ref.search(S, graph, seeds, k, ef, 200)
            for q in range(Q):
                got = i[q].tolist()
                assert len(set(got)) == k and min(got) >= 0, (ef, k, q)              # no row twice, no pad
                assert got == sorted(got, key=lambda r: ref.beam_key(S[q, r], r)), (ef, k, q)
                assert (v[q].view(np.int32) == S[q, got].view(np.int32)).all()       # each with its own bits (the sign of a zero too)
    # the whole graph in the beam: the exhaustive order, every rule visible
    v, i, iters, visited = ref.search(S, graph, seeds, G, G, 200)
    assert (visited == G).all() and (iters == G).all()
    for q in range(Q):
        wv, wi = ref.topk_exact(S[q], G)
        assert (i[q] == wi).all() and (v[q].view(np.int32) == wv.view(np.int32)).all()
    assert i[0, 0] == 7 and i[1, :3].tolist() == [7, 37, 52]             # NaN first, the lower row first among them
    order = i[2].tolist()
    zeros = [r for r in order if S[2, r] == 0]
    assert zeros == [10, 11, 12, 13, 40, 41, 42, 43]                     # -0 = +0: by row alone
    assert all(order.index(r) + 1 == order.index(r + 30) for r in range(30) if r not in range(10, 14))    # a copy follows its original
    assert i[3].tolist() == [20] + [r for r in range(G) if r != 20]
    # a beam of two among the eight zeros of query 3: the two lowest rows seen stay, whatever comes later
    v, i, iters, visited = ref.search(S[3:], graph, np.array([[45, 2]]), 2, 2, 200)
    # 2 -> 3 1 32 9 (45 drops out), 1 -> 0 31 8, 0 -> 59 30 7: nothing below row 0 is left to find
    assert i[0].tolist() == [0, 1] and iters[0] == 3 and visited[0] == 12


def test_one_iteration_expands_one_row():
    G = 30
    graph = np.stack([[(r + 1) % G, (r + 2) % G, (r + 7) % G] for r in range(G)]).astype(np.int32)
    S = np.linspace(0.0, 1.0, G, dtype=np.float32)[None, :]
    v, i, iters, visited = ref.search(S, graph, np.array([[4, 10, -1, 4]]), 5, 8, 1)
    # the seeds 4 and 10 (-1 and the repeat skipped); 10 is the better one and is expanded: 11, 12, 17
    assert iters[0] == 1 and visited[0] == 5 and i[0].tolist() == [17, 12, 11, 10, 4]
    v, i, iters, visited = ref.search(S, graph, np.array([[4, 10, -1, 4]]), 2, 2, 1)
    assert i[0].tolist() == [17, 12] and visited[0] == 5                 # a row that dropped out of the beam stays visited


def test_beam_stops_when_every_entry_is_expanded():
    G = 40
    graph = np.stack([[(r + 1) % G, (r - 1) % G] for r in range(G)]).astype(np.int32)
    S = -np.abs(np.arange(G, dtype=np.float32) - 20.0)[None, :]          # one peak at row 20
    v, i, iters, visited = ref.search(S, graph, np.array([[3]]), 3, 4, 1000)
    assert i[0].tolist() == [20, 19, 21]
    # the walk climbs from 3 to 20, goes on until the 4 best are expanded and stops well before max_iters
    assert 17 < iters[0] < 30 and visited[0] < G


def test_a_disconnected_component_is_never_reached():
    G = 20
    graph = np.stack([[(r + 1) % 10 + 10 * (r // 10), (r + 3) % 10 + 10 * (r // 10)] for r in range(G)]).astype(np.int32)
    S = np.arange(G, dtype=np.float32)[None, :]                          # the best rows are all in the second component
    v, i, iters, visited = ref.search(S, graph, np.array([[0, 5]]), 4, 16, 100)
    assert i[0].tolist() == [9, 8, 7, 6] and visited[0] == 10 and iters[0] == 10
    v, i, _, _ = ref.search(S, graph, np.array([[0, 5]]), 12, 16, 100)
    assert (i[0, :10] < 10).all() and (i[0, 10:] == -1).all() and np.isneginf(v[0, 10:]).all()


def test_filter_chooses_among_the_beam_and_never_changes_the_walk():
    rng = np.random.default_rng(3)
    G, Q = 50, 4
    graph = rng.integers(-1, G, (G, 6)).astype(np.int32)
    S = rng.standard_normal((Q, G)).astype(np.float32)
    seeds = rng.integers(0, G, (Q, 3))
    glab, qlab, ex = rng.integers(0, 3, G), rng.integers(0, 3, Q), np.array([107, -1, 100, 149])
    plain = ref.search(S, graph, seeds, 12, 12, 20)                      # k = ef: the whole beam
    el =ref.eligible_mask(Q, G, qlab, glab, "different", ex, idx_offset=100)
    filt = ref.search(S, graph, seeds, 10, 12, 20, el, idx_offset=100)
    assert (filt[2] == plain[2]).all() and (filt[3] == plain[3]).all()
    for q in range(Q):
        want = [int(r) + 100 for r in plain[1][q] if r >= 0 and glab[r] != qlab[q] and r + 100 != ex[q]][:10]
        assert filt[1][q, : len(want)].tolist() == want and (filt[1][q, len(want):] == -1).all()


def test_an_id_outside_the_rows_raises():
    S = np.zeros((1, 5), np.float32)
    graph = np.array([[1, 2], [2, 3], [3, 4], [4, 0], [0, 5]], np.int32)
    with pytest.raises(ValueError):
        ref.search(S, graph, np.array([[5]]), 1, 2, 3)
    with pytest.raises(ValueError):
        ref.search(S, graph, np.array([[-2]]), 1, 2, 3)
    with pytest.raises(ValueError):
        ref.search(S, graph, np.array([[0]]), 1, 8, 10)                  # the walk reaches row 4, whose list names row 5
    assert ref.search(S, graph, np.array([[0]]), 1, 8, 2)[2][0] == 2     # ... and stops short of it within two expansions


def _brute_merged(fwd, degree):
    G, h = fwd.shape
    out = np.full((G, degree), -1, np.int32)
    out[:, :h] = fwd
    for r in range(G):
        cand = []
        for s in range(G):
            pos = [p for p in range(h) if fwd[s, p] == r]
            if pos and s not in fwd[r]:
                cand.append((pos[0], s))
        keep = [s for _, s in sorted(cand)][: degree - h]
        out[r, h: h + len(keep)] = keep
    return out


@pytest.mark.parametrize("G,h,lo", [(1, 1, 0), (7, 1, 0), (40, 3, -1), (200, 4, 0), (64, 8, -1), (150, 32, 0)])
def test_merged_graph_model_and_torch_sorts_agree_with_brute_force(G, h, lo):
    rng = np.random.default_rng(G + h)
    fwd = rng.integers(lo, G, (G, h))                                    # pads (-1), self-loops and repeats all occur
    if G > 20:
        fwd[:, 0] = 3                                                    # one popular row: its reverse list is cut
    want = _brute_merged(fwd, 2 * h)
    assert (ref.merged_graph(fwd, 2 * h) == want).all()
    got = graph.merged_graph(torch.from_numpy(fwd), 2 * h)
    assert got.dtype == torch.int32 and (got.numpy() == want).all()
    if G > 20:
        assert (want[3, h:] >= 0).all() and (want[:, h:] == -1).any()


def test_merged_graph_refusals():
    f = torch.zeros((5, 2), dtype=torch.int64)
    for degree in (3, 0, 66, 2.0, True, None):
        with pytest.raises(MI355Error, match="degree"):
            graph.merged_graph(f, degree)
    with pytest.raises(MI355Error, match="fwd must be"):
        graph.merged_graph(f, 6)
    with pytest.raises(MI355Error, match="integers"):
        graph.merged_graph(f.float(), 4)
