"""Full-gallery ranks, mAP and CMC on the GPU.  The expected value is the CPU reference (tests/ranking_ref.py) applied to the
library's own score slab (``cosine_scores`` on the same path, or an fp16 gallery's own search): ranks and first ranks must match
exactly, the average precision bit for bit (same summation order).  Shapes sit on the tile edges (128 gallery rows, 64 / 128
query rows), both GEMM loops, every class size from none to 1100, massive ties, same-source, idx_offset, NaN rows, fp16, several
query blocks; then an independent float64 check on well-separated queries."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import lib
from imageretrievalresearch_amd import rank as R

import ranking_ref as RR
from helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLIT, EXACT, F16_GEMM = 2, 3, 5


def _randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


def _labels(n, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, classes, (n,), generator=g).to(DEV)


def _tiled_scores(q, g, **kw):
    """The slab of q against g on the tiled GEMM: queries padded to 8 rows (Q <= 4 would take the GEMV, whose bits differ)."""
    Q = q.shape[0]
    if Q > 4:
        return M.cosine_scores(q, g, **kw)
    pad = torch.cat([q, torch.ones((8 - Q, q.shape[1]), device=q.device)])
    return M.cosine_scores(pad, g, **kw)[:Q].contiguous()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _assert_matches(got, S, ql, gl, exclude=None, idx_offset=0, what=""):
    """got = (PositiveRanks, ap, first_rank) against the reference on the slab S; returns the reference."""
    pr, ap, first = got
    ref = RR.rank_positives(_np(S), _np(ql), _np(gl), _np(exclude), idx_offset)
    off, idx, ranks, ap_ref, first_ref = ref
    assert pr.offsets.dtype == pr.indices.dtype == pr.ranks.dtype == first.dtype == torch.int64
    assert pr.scores.dtype == torch.float32 and ap.dtype == torch.float64
    assert np.array_equal(_np(pr.offsets), off), what
    assert np.array_equal(_np(pr.indices), idx), what
    assert np.array_equal(_np(pr.ranks), ranks), what
    assert np.array_equal(_np(first), first_ref), what
    assert np.array_equal(_np(ap), ap_ref), (what, np.abs(_np(ap) - ap_ref).max())      # same summation order: same bits
    qi = np.repeat(np.arange(S.shape[0]), np.diff(off))
    want = _np(S)[qi, idx - idx_offset]
    assert np.array_equal(_np(pr.scores).view(np.int32), want.view(np.int32)), what      # the slab's bits
    return ref


def _ranks(q, ql, g, gl, exclude=None, idx_offset=0, **kw):
    return R._positive_ranks(q, ql, R._Rows.of(g), gl, exclude, idx_offset, **kw)


def run_case(Q, G, D, path, seed=0):
    """One random case with a handful of classes and a random exclusion; ``path``: the GEMM loop it must take."""
    q, g = _randn((Q, D), seed + 1), _randn((G, D), seed + 2)
    ql, gl = _labels(Q, 5, seed + 3), _labels(G, 6, seed + 4)           # (label 5: gallery only)
    ex = torch.randint(0, G, (Q,), generator=torch.Generator().manual_seed(seed + 5)).to(DEV)
    ex[::3] = -1
    got = _ranks(q, ql, g, gl, ex)
    assert lib().mi355_rank_last_path() == path
    _assert_matches(got, _tiled_scores(q, g), ql, gl, ex, what=(Q, G, D))


# ---------------------------------------------------------------- 1. tile edges, both loops
@pytest.mark.parametrize("G", [127, 128, 129, 257])
@pytest.mark.parametrize("Q", [3, 64, 65, 130])
def test_tile_edges(Q, G):
    run_case(Q, G, 48, SPLIT, seed=Q * 1000 + G)


@pytest.mark.parametrize("Q,G", [(3, 129), (65, 257), (130, 128)])
def test_exact_f32_loop_for_unaligned_dim(Q, G):
    run_case(Q, G, 70, EXACT, seed=7)


def test_exact_f32_loop_by_environment_in_a_fresh_process():
    child = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]\n"
             "import test_ranking_metrics_gpu as T\n"
             "T.run_case(65, 257, 48, T.EXACT, seed=11)\n"
             "T.run_case(130, 129, 48, T.EXACT, seed=12)\n"
             "print('child ok')\n")
    env = dict(os.environ, MI355_RANK_EXACT_F32="1")
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- 2. class sizes: none, 1, 2, 200, 1100
def test_class_sizes_up_to_1100_where_retrieval_accuracy_refuses():
    Q, G, D = 8, 1500, 32
    sizes = {0: 1100, 1: 200, 2: 2, 3: 1, 4: G - 1303}
    lab = torch.cat([torch.full((n,), c) for c, n in sizes.items()])
    gl = lab[torch.randperm(G, generator=torch.Generator().manual_seed(21))].to(DEV)     # every class spread over the tiles
    ql = torch.tensor([0, 1, 2, 3, 99, 0, 1, 4], device=DEV)                             # 99: a lone query
    q, g = _randn((Q, D), 22), _randn((G, D), 23)
    with pytest.raises(M.MI355Error, match="retrieval_accuracy ranks at most 1024"):
        M.retrieval_accuracy(q, ql, g, gl)
    m = M.ranking_metrics(q, ql, g, gl)
    assert m["R"].tolist() == [1100, 200, 2, 1, 0, 1100, 200, G - 1303] and int(m["num_lone"]) == 1
    ref = _assert_matches((m["positive_ranks"], m["per_query_ap"], m["first_rank"]), _tiled_scores(q, g), ql, gl)
    assert ref[4][4] == 0 and float(m["per_query_ap"][4]) == 0.0
    # the whole class is ranked: the last positive of the 1100 sits beyond any top-k the library has
    pr = m["positive_ranks"]
    assert int(pr.ranks[pr.offsets[1] - 1]) > 1100 and 0.0 < float(m["map"]) < 1.0


# ---------------------------------------------------------------- 3. ties
def _tie_rows(n_each, seed):
    base = torch.tensor([[1, 2, 0, -1, 3, 0, 1, 2], [2, -1, 1, 0, 0, 3, 1, -2], [0, 1, 1, 2, -2, 1, 0, 3],
                         [3, 0, -1, 1, 2, 2, 0, 1], [1, 1, 2, 0, 1, -1, 3, 0]], dtype=torch.float32)
    ids = torch.arange(5).repeat_interleave(n_each)
    ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(seed))]
    return base[ids].to(DEV), ids.to(DEV)


def test_massive_ties_resolve_to_the_lower_row():
    g, gl = _tie_rows(60, 31)                                   # 5 distinct vectors x 60, shuffled
    q, ql = _tie_rows(4, 32)
    S = _tiled_scores(q, g)
    assert all(torch.unique(S[i]).numel() <= 5 for i in range(q.shape[0]))               # the slab really ties
    pr, ap, first = got = _ranks(q, ql, g, gl)
    _assert_matches(got, S, ql, gl)
    # every query's 60 positives are its own duplicates: one score, rows ascending, ranks 1 .. 60
    for i in range(q.shape[0]):
        seg = slice(int(pr.offsets[i]), int(pr.offsets[i + 1]))
        assert torch.unique(pr.scores[seg]).numel() == 1
        assert torch.equal(pr.indices[seg], torch.nonzero(gl == ql[i]).flatten())
        assert torch.equal(pr.ranks[seg], torch.arange(1, 61, device=DEV))
    assert torch.equal(ap, torch.ones_like(ap)) and torch.equal(first, torch.ones_like(first))
    # split every vector's duplicates into two classes by row parity: now each query's positives tie with NEGATIVES (the
    # same vector under the other label), interleaved by row: every such tie must go to the lower row
    gl2, ql2 = gl * 2 + torch.arange(g.shape[0], device=DEV) % 2, ql * 2
    pos, neg = S[0][gl2 == ql2[0]], S[0][gl2 == ql2[0] + 1]
    assert pos.numel() > 10 and neg.numel() > 10 and torch.unique(torch.cat([pos, neg])).numel() == 1
    pr2, ap2, first2 = got2 = _ranks(q, ql2, g, gl2)
    _assert_matches(got2, S, ql2, gl2)
    dup = torch.nonzero(gl == ql[0]).flatten()                  # the 60 tied rows of query 0, ascending: rank = position + 1
    want = torch.nonzero(gl2[dup] == ql2[0]).flatten() + 1
    assert torch.equal(pr2.ranks[: want.numel()], want) and float(ap2[0]) < 1.0


def test_same_source_excludes_the_own_row_and_keeps_its_duplicates():
    x, lab = _tie_rows(30, 41)                                  # G = Q = 150: every row has 29 exact duplicates
    S = _tiled_scores(x, x)
    ex = torch.arange(150, device=DEV)
    pr = M.positive_ranks(x, lab)
    m = M.ranking_metrics(x, lab)
    assert torch.equal(pr.ranks, m["positive_ranks"].ranks) and torch.equal(pr.indices, m["positive_ranks"].indices)
    _assert_matches((pr, m["per_query_ap"], m["first_rank"]), S, lab, lab, ex)
    assert (pr.offsets[1:] - pr.offsets[:-1] == 29).all()
    rows = torch.arange(150, device=DEV).repeat_interleave(29)
    assert not (pr.indices == rows).any()                        # never the own row
    with pytest.raises(M.MI355Error, match="same-source"):
        M.positive_ranks(x, lab, exclude=ex)


# ---------------------------------------------------------------- 4. idx_offset, NaN
def test_idx_offset_with_global_exclude():
    Q, G, D, off = 70, 300, 48, 100000
    q, g = _randn((Q, D), 51), _randn((G, D), 52)
    ql, gl = _labels(Q, 4, 53), _labels(G, 4, 54)
    best = _tiled_scores(q, g).masked_fill(ql[:, None] != gl[None, :], -2.0).argmax(1)   # each query's best positive
    ex = best + off
    ex[::4] = -1
    ex[1] = 5                                                    # a row of another shard: excludes nothing
    pr = M.positive_ranks(q, ql, g, gl, exclude=ex, idx_offset=off)
    got = _ranks(q, ql, g, gl, ex, off)
    assert all(torch.equal(a, b) for a, b in zip(pr, got[0]))
    _assert_matches(got, _tiled_scores(q, g), ql, gl, ex, off)
    assert int(pr.indices.min()) >= off and not (pr.indices[pr.offsets[2]:pr.offsets[3]] == ex[2]).any()


def test_nan_rows_rank_first_as_negative_and_as_positive():
    Q, G, D = 66, 200, 48
    q, g = _randn((Q, D), 61), _randn((G, D), 62)
    ql, gl = _labels(Q, 3, 63), _labels(G, 3, 64)
    g[5] = float("nan")
    g[130, 7] = float("nan")
    gl[5], gl[130] = 0, 1
    ql[0], ql[1] = 0, 1                                          # row 5 is query 0's positive, row 130 query 1's
    S = _tiled_scores(q, g)
    assert bool(torch.isnan(S[:, 5]).all()) and bool(torch.isnan(S[:, 130]).all())
    got = _ranks(q, ql, g, gl)
    _assert_matches(got, S, ql, gl)
    pr, ap, first = got
    assert int(first[0]) == 1 and int(pr.indices[pr.offsets[0]]) == 5                    # NaN above every number, lower row first
    assert int(first[1]) == 2 and int(pr.indices[pr.offsets[1]]) == 130
    assert bool(torch.isnan(pr.scores[pr.offsets[0]])) and bool(torch.isnan(pr.scores[pr.offsets[1]]))
    third = int(torch.nonzero(ql == 2)[0])                       # both NaN rows are negatives: every rank is pushed by two
    assert int(first[third]) >= 3


# ---------------------------------------------------------------- 5. resident galleries
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_gallery_method_against_its_own_slab(dtype):
    Q, G, D = 37, 300, 100
    q, x = _randn((Q, D), 71), _randn((G, D), 72)
    ql, gl = _labels(Q, 5, 73), _labels(G, 5, 74)
    gal = M.Gallery(D, DEV, dtype=dtype).add(x, gl)
    if dtype == torch.float16:
        v, i = gal.search(q, G)                                  # every row, descending (the tiled kernel's slab, k > 8)
        S = torch.empty((Q, G), device=DEV).scatter_(1, i, v)
    else:
        S = M.cosine_scores(q, gal.data, gallery_is_normalized=True)
    ex = torch.randint(-1, G, (Q,), generator=torch.Generator().manual_seed(75)).to(DEV)
    m = gal.ranking_metrics(q, ql, exclude=ex, ranks=(1, 3))
    assert lib().mi355_rank_last_path() == (F16_GEMM if dtype == torch.float16 else SPLIT)
    _assert_matches((m["positive_ranks"], m["per_query_ap"], m["first_rank"]), S, ql, gl, ex)
    assert sorted(m["cmc"]) == [1, 3]
    with pytest.raises(M.MI355Error, match="needs gallery labels"):
        M.Gallery(D, DEV, dtype=dtype).add(x).ranking_metrics(q, ql)


# ---------------------------------------------------------------- 6. query blocks, determinism
def test_query_blocks_and_two_runs_are_bit_identical():
    Q, G, D = 130, 257, 48
    q, g = _randn((Q, D), 81), _randn((G, D), 82)
    ql, gl = _labels(Q, 4, 83), _labels(G, 4, 84)
    one = _ranks(q, ql, g, gl)
    _assert_matches(one, _tiled_scores(q, g), ql, gl)
    for kw in (dict(block=64), dict(block=1000), dict()):        # 3 blocks (64 + 64 + 2), one block, again
        other = _ranks(q, ql, g, gl, **kw)
        for a, b in zip(tuple(one[0]) + one[1:], tuple(other[0]) + other[1:]):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), kw
    with pytest.raises(M.MI355Error, match="block"):
        _ranks(q, ql, g, gl, block=0)


# ---------------------------------------------------------------- 7. aggregates, consistency with retrieval_accuracy
def test_aggregates_equal_host_means_of_the_per_query_outputs():
    Q, G, D = 90, 400, 48
    q, g = _randn((Q, D), 91), _randn((G, D), 92)
    ql, gl = _labels(Q, 8, 93), _labels(G, 6, 94)               # labels 6, 7: lone queries
    m = M.ranking_metrics(q, ql, g, gl, ranks=(1, 5, 10, 20))
    R_, ap, first = _np(m["R"]), _np(m["per_query_ap"]), _np(m["first_rank"])
    valid = R_ > 0
    assert m["num_queries"] == Q and int(m["num_lone"]) == int((~valid).sum()) > 0
    # the mean of Q float64 terms in [0, 1], summed in whatever order the device reduces them: each partial sum rounds once,
    # so it lies within (Q - 1) * 2^-53 (relative) of the exact sum (math.fsum), and the division rounds once more
    exact = math.fsum(ap[valid].tolist()) / int(valid.sum())
    assert abs(float(m["map"]) - exact) <= Q * 2.0 ** -53 * exact
    assert float(m["mean_first_rank"]) == float((first * valid).sum() / valid.sum())
    assert sorted(m["cmc"]) == [1, 5, 10, 20]
    for r in (1, 5, 10, 20):
        assert float(m["cmc"][r]) == RR.cmc(first, R_, r)
    assert (ap[~valid] == 0).all() and (first[~valid] == 0).all()
    assert float(m["cmc"][1]) <= float(m["cmc"][5]) <= float(m["cmc"][10]) <= float(m["cmc"][20]) <= 1.0


def test_consistent_with_retrieval_accuracy_on_a_random_case():
    N, D = 200, 32
    x, lab = _randn((N, D), 101), _labels(N, 10, 102)
    ks = (1, 2, 4, 8)
    acc = M.retrieval_accuracy(x, lab, ks=ks)
    m = M.ranking_metrics(x, lab, ranks=ks)
    assert float(m["cmc"][1]) == float(acc["precision_at_1"])
    for K in ks:
        assert float(m["cmc"][K]) == float(acc["recall_at_k"][K])
    assert int(m["num_lone"]) == int(acc["num_lone"]) and torch.equal(m["R"], acc["R"])
    # MAP@R looks at the first R_q ranks only: never above the full-gallery AP
    assert float(acc["map_at_r"]) <= float(m["map"])


def test_query_expansion_ranks_the_expanded_queries():
    N, D = 150, 48
    x, lab = _randn((N, D), 111), _labels(N, 6, 112)
    ex = torch.arange(N, device=DEV)
    m = M.ranking_metrics(x, lab, query_expansion=(3, 2.0))
    xq = M.expand_queries(x, x, 3, 2.0, exclude=ex)
    got = _ranks(xq, lab, x, lab, ex)
    assert torch.equal(m["positive_ranks"].ranks, got[0].ranks) and torch.equal(m["per_query_ap"], got[1])
    _assert_matches(got, _tiled_scores(xq, x), lab, lab, ex)


# ---------------------------------------------------------------- 8. independent float64 check
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_ranks_against_the_float64_oracle_on_separated_queries(seed):
    """Expected ranks from float64 scores (oracle/rank.py's normalise-then-dot).  A query is left out only if, in float64, one
    of its positives lies within 2e-5 of another eligible row: twice the project's 1e-5 score tolerance, since either score
    may move by that much.  At most 25 % of the queries may be left out; for every other one the ranks match exactly."""
    from oracle import rank as O
    Q, G, D = 32, 200, 64
    rng = np.random.default_rng(seed)
    qn, gn = rng.standard_normal((Q, D)).astype(np.float32), rng.standard_normal((G, D)).astype(np.float32)
    gl = np.arange(G) % 50
    ql = rng.integers(0, 50, Q)
    S64 = O.l2_normalize_rows(qn).astype(np.float64) @ O.l2_normalize_rows(gn).astype(np.float64).T
    pr = M.positive_ranks(torch.from_numpy(qn).to(DEV), torch.from_numpy(ql).to(DEV), torch.from_numpy(gn).to(DEV),
                          torch.from_numpy(gl).to(DEV))
    off, idx, ranks = _np(pr.offsets), _np(pr.indices), _np(pr.ranks)
    assert np.array_equal(np.diff(off), np.full(Q, 4))
    kept = 0
    for i in range(Q):
        pos = np.nonzero(gl == ql[i])[0]
        gap = np.abs(S64[i][None, :] - S64[i, pos][:, None])
        gap[np.arange(pos.size), pos] = np.inf
        if gap.min() <= 2e-5:
            continue
        kept += 1
        order = np.argsort(-S64[i], kind="stable")
        where = np.nonzero(gl[order] == ql[i])[0]
        assert np.array_equal(idx[off[i]:off[i + 1]], order[where]), (seed, i)
        assert np.array_equal(ranks[off[i]:off[i + 1]], where + 1), (seed, i)
    print(f"seed {seed}: {Q - kept} of {Q} queries left out")
    assert Q - kept <= Q // 4
