"""The selection kernels of csrc/rank.hip, directly and exactly, at the edges of their chunks, levels and slabs: k_topk_small<K>,
k_topk_bitonic, the level loop and the 65535-row slab loop of topk_select (through M.topk / M.merge_topk),
k_pack_candidates / k_unpack_candidates (rank.pack_candidates / rank.merge_packed_topk), k_clear_pads, k_hit_counts and
k_distinct_topn.  The reference is tests/select_ref.py; every comparison is an equality.

Shapes follow the constants of rank.hip / rank_common.h: SMALL_K = 8 (k <= 8: per-thread lists over chunks of
SMALL_CHUNK = 8192, templates K = 1, 2, 4, 8), BT_N = 2048 (k > 8: one bitonic sort per chunk), each level leaving
chunks * k candidates to the next, and the grid.y slab of 65535 rows."""
import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import rank
import select_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_CHUNK, BT_N, SLAB = 8192, 2048, 65535
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.cpu().numpy()


def pattern_rows(n, k, chunk, seed):
    """One row per value pattern, (rows, n) float32: (a) distinct, (b) four levels, (c) all equal, (d) ascending and
    descending, (e) the k largest in the last n % chunk elements, (f) -inf everywhere but a +inf, both zeros and one
    finite value, (g) more NaNs than k and exactly one NaN (in the last chunk)."""
    rng = np.random.default_rng(seed)
    rows = []
    a = rng.permutation(n).astype(np.float32) - np.float32(n // 2)
    rows.append(a)                                                              # (a)
    rows.append(rng.integers(0, 4, n).astype(np.float32) * np.float32(0.25))    # (b)
    rows.append(np.full(n, 0.25, np.float32))                                   # (c)
    rows.append(np.arange(n, dtype=np.float32))                                 # (d)
    rows.append(-np.arange(n, dtype=np.float32))
    tail = min(n, (n % chunk) or chunk)
    e = rng.permutation(n).astype(np.float32)
    m = min(k, tail)
    e[n - tail + rng.choice(tail, m, replace=False)] = np.float32(n) + rng.permutation(m).astype(np.float32) + 1
    rows.append(e)                                                              # (e)
    f = np.full(n, -INF, np.float32)
    f[n // 2], f[(3 * n) // 4], f[n // 3], f[n - 1] = -1.5, -0.0, 0.0, INF
    rows.append(f)                                                              # (f)
    g = a.copy()
    g[rng.choice(n, min(n, k + 3), replace=False)] = NAN
    rows.append(g)                                                              # (g)
    g = a.copy()
    g[n - 1 - (tail // 2)] = NAN
    rows.append(g)
    return np.stack(rows)


def check_topk(S, k, idx_offset=0, what=""):
    """M.topk of the slab S against the reference: indices, values, and every value the input's own bits at its index."""
    v, i = M.topk(dev(S), k, idx_offset=idx_offset)
    v, i = host(v), host(i)
    want_v, want_i = R.select_topk(S, None, k, idx_offset)
    R.assert_selection_equal(v, i, want_v, want_i, what)
    src = np.take_along_axis(S, i - idx_offset, 1)
    np.testing.assert_array_equal(R.bits(v), R.bits(src), err_msg=f"{what}: value bits")


# ---- k <= 8: k_topk_small<1|2|4|8>, chunks of 8192; 8193 and 16385 run two levels
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8])
@pytest.mark.parametrize("rowlen", ["k", 255, 256, 257, 8191, 8192, 8193, 16385])
def test_small_k_chunk_edges(k, rowlen):
    n = k if rowlen == "k" else rowlen
    S = pattern_rows(n, k, SMALL_CHUNK, 1000 * k + n)
    check_topk(S, k, idx_offset=2 ** 32 + 11 if n == 8193 else 0, what=f"small k={k} n={n}")


def test_small_k_three_levels():
    """8 388 609 = 1024 * 8192 + 1 columns at k = 8: 1025 level-1 chunks -> 8200 candidates -> 2 chunks -> 16 -> k.  The
    last column is a chunk of its own at level 1 and the second chunk's only list at level 2."""
    n, k = 1024 * SMALL_CHUNK + 1, 8
    rng = np.random.default_rng(77)
    a = rng.permutation(n).astype(np.float32)                 # (a) distinct (integers below 2^24: exact)
    top = np.argmax(a)
    a[top], a[n - 1] = a[n - 1], a[top]                       # the maximum in the last, one-element chunk
    b = rng.integers(0, 3, n).astype(np.float32) * np.float32(0.25)       # (b) four levels, the top one at six columns
    b[[SMALL_CHUNK - 1, SMALL_CHUNK, 4_000_000, 1023 * SMALL_CHUNK + 5, n - 2, n - 1]] = 0.75
    S = np.stack([a, b])
    v, i = M.topk(dev(S), k)
    v, i = host(v), host(i)
    for r in range(2):
        row = S[r]
        t = np.partition(row, n - k)[n - k]                   # the k-th largest value
        keep = np.sort(np.concatenate([np.flatnonzero(row > t), np.flatnonzero(row == t)[:k]]))
        want_v, want_i = R.select_topk(row[keep][None], keep[None].astype(np.int64), k)
        R.assert_selection_equal(v[r:r + 1], i[r:r + 1], want_v, want_i, f"three levels row {r}")
        np.testing.assert_array_equal(R.bits(v[r]), R.bits(row[i[r]]))
    assert i[0, 0] == n - 1 and i[1].tolist()[:6] == [SMALL_CHUNK - 1, SMALL_CHUNK, 4_000_000, 1023 * SMALL_CHUNK + 5, n - 2, n - 1]


# ---- k > 8: k_topk_bitonic, chunks of 2048; 4097 at k = 1024 runs three levels (3 chunks -> 3072 -> 2 chunks -> 2048 -> k)
BITONIC = [(k, n) for k in (9, 255, 256, 257, 1023, 1024) for n in ("k", 2047, 2048, 2049, 4097, 10241)
           if n == "k" or k <= n]


@pytest.mark.parametrize("k,rowlen", BITONIC)
def test_bitonic_chunk_edges(k, rowlen):
    n = k if rowlen == "k" else rowlen
    S = pattern_rows(n, k, BT_N, 2000 * k + n)
    check_topk(S, k, idx_offset=2 ** 32 + 11 if n == 2049 else 0, what=f"bitonic k={k} n={n}")


# ---- the grid.y slab loop of topk_select: rows past 65535 read and write at their own offsets
@pytest.mark.parametrize("Q", [SLAB, SLAB + 1, SLAB + 6])
@pytest.mark.parametrize("rowlen,k", [(9, 3), (12, 9)])
def test_query_slabs(Q, rowlen, k):
    q = np.arange(Q)
    S = np.tile(-np.arange(rowlen, dtype=np.float32) - 1, (Q, 1))
    S[q, (q + 2) % rowlen] = 50.0                             # a tie pair
    S[q, (q + 5) % rowlen] = 50.0
    S[q, q % rowlen] = (1000 + q).astype(np.float32)          # the row's own maximum, at its own column
    check_topk(S, k, what=f"slabs Q={Q} n={rowlen} k={k}")


# ---- mi355_merge_topk: explicit int64 indices
def merge_rows(ncand, k, seed):
    """Candidate rows (values, shuffled global ids, some above 2^31): all real and distinct; four levels; some candidates
    marked missing (int64 max) with values that would win; fewer than k real ones among int64-max and (-inf, 1 << 62)
    entries; real -inf candidates next to (-inf, 1 << 62) pads."""
    rng = np.random.default_rng(seed)
    ids = lambda: rng.choice(2 ** 34, ncand, replace=False).astype(np.int64)       # noqa: E731
    V, I = [], []
    V.append(rng.permutation(ncand).astype(np.float32)); I.append(ids())
    V.append(rng.integers(0, 4, ncand).astype(np.float32) * np.float32(0.25)); I.append(ids())
    v, i = rng.permutation(ncand).astype(np.float32), ids()
    gone = rng.choice(ncand, max(1, ncand // 3), replace=False)
    v[gone[::2]] = 9e9
    i[gone] = R.IDX_PAD
    V.append(v); I.append(i)
    v, i = rng.integers(0, 3, ncand).astype(np.float32), ids()
    fake = rng.permutation(ncand)[: ncand - max(1, k // 2)]
    i[fake[::2]] = R.IDX_PAD
    v[fake[::2]] = INF
    i[fake[1::2]] = 2 ** 62
    v[fake[1::2]] = -INF
    V.append(v); I.append(i)
    v, i = np.full(ncand, -INF, np.float32), ids()
    i[rng.permutation(ncand)[: ncand // 2]] = 2 ** 62
    v[0] = NAN
    V.append(v); I.append(i)
    return np.stack(V), np.stack(I)


@pytest.mark.parametrize("k,ncand", [(3, 3), (3, 9), (8, 8), (8, 24), (8, 8193), (9, 9), (9, 27), (1024, 1024), (1024, 3072)])
def test_merge_topk(k, ncand):
    """A candidate whose index is >= 2^62 (int64 max, or the shard pad 1 << 62) is no candidate: its value is ignored and
    the slots that stay empty come back as (-inf, int64 max), on the small-k and the bitonic path alike."""
    V, I = merge_rows(ncand, k, 31 * k + ncand)
    v, i = M.merge_topk(dev(V), dev(I), k)
    v, i = host(v), host(i)
    want_v, want_i, pos = R.select_topk(V, I, k, return_pos=True)
    R.assert_selection_equal(v, i, want_v, want_i, f"merge k={k} ncand={ncand}")
    src = np.where(pos >= 0, np.take_along_axis(V, np.maximum(pos, 0), 1), -INF)
    np.testing.assert_array_equal(R.bits(v), R.bits(src))
    assert (want_i[3] == R.IDX_PAD).sum() == k - max(1, k // 2)       # the row with fewer than k real candidates has pads


# ---- mi355_pack_candidates
@pytest.mark.parametrize("k,kk", [(1, 0), (1, 1), (5, 0), (5, 1), (5, 4), (5, 5)])
def test_pack_candidates_bits(k, kk):
    Q = 3
    rng = np.random.default_rng(k * 10 + kk)
    vals = rng.standard_normal((Q, kk)).astype(np.float32)
    idx = rng.integers(0, 2 ** 31 - 1, (Q, kk)).astype(np.int64)
    if kk:
        vals.view(np.uint32)[0, 0] = 0x7FC12345               # a NaN with a payload
        vals[1, kk - 1] = -0.0
        vals[2, 0] = -INF
        idx[2, 0] = 2 ** 31 - 1
    got = rank.pack_candidates(dev(vals) if kk else None, dev(idx) if kk else None, Q, k, DEV)
    want = R.pack(vals if kk else None, idx if kk else None, Q, k)
    assert got.dtype == torch.int32 and tuple(got.shape) == (Q, k, 2)
    np.testing.assert_array_equal(host(got), want)
    assert (want[:, kk:, 0].view(np.uint32) == 0xFF800000).all() and (want[:, kk:, 1] == -1).all()


# ---- mi355_merge_packed_topk
def ragged_sizes(world, k):
    """Rows per shard: unequal, one empty, one with fewer rows than k (where world and k leave room for it)."""
    return {1: [max(1, k // 2)], 2: [0, max(1, k // 2)], 3: [k + 5, 0, max(1, k - 1)],
            7: [k + 5, 0, max(1, k // 2), 2 * k, 1, k, k + 1]}[world]


def packed_shards(sizes, k, Q, seed):
    """Each shard's local top-min(k, rows) of its own four-level scores, packed on the GPU (and checked against the
    reference's packing); the offsets of consecutive shards, the first at 2^33 + 5."""
    rng = np.random.default_rng(seed)
    packed, lists = [], []
    for rows in sizes:
        kk = min(k, rows)
        if kk:
            S = rng.integers(0, 4, (Q, rows)).astype(np.float32) * np.float32(0.25)
            S[0, rows // 2] = NAN
            lv, li = R.select_topk(S, None, kk)
            p = rank.pack_candidates(dev(lv), dev(li), Q, k, DEV)
        else:
            lv = li = None
            p = rank.pack_candidates(None, None, Q, k, DEV)
        np.testing.assert_array_equal(host(p), R.pack(lv, li, Q, k))
        packed.append(p)
        lists.append((lv, li))
    offsets = 2 ** 33 + 5 + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return torch.stack(packed), offsets, lists


@pytest.mark.parametrize("world", [1, 2, 3, 7])
@pytest.mark.parametrize("k", [1, 3, 8, 9, 150, 1024])
def test_merge_packed_topk(world, k):
    """A slot that no shard fills comes back as (-inf, int64 max); ShardedGallery turns it into (-inf, -1) with clear_pads
    over [0, total rows), as the last step here does."""
    Q = 3
    # ragged shards
    sizes = ragged_sizes(world, k)
    packed, offsets, _ = packed_shards(sizes, k, Q, 7 * world + k)
    v, i = rank.merge_packed_topk(packed, dev(offsets), k)
    want_v, want_i = R.unpack_merge(host(packed), offsets, k)
    R.assert_selection_equal(host(v), host(i), want_v, want_i, f"packed world={world} k={k}")
    np.testing.assert_array_equal(R.bits(host(v)), R.bits(want_v))
    assert (want_i == R.IDX_PAD).sum() == Q * max(0, k - sum(sizes))
    lo, hi = int(offsets[0]), int(offsets[0]) + sum(sizes)
    cv, ci = rank.clear_pads(v, i, lo, hi)
    want_cv, want_ci = R.clear_pads(want_v, want_i, lo, hi)
    R.assert_selection_equal(host(cv), host(ci), want_cv, want_ci, "after clear_pads")
    assert (want_ci == -1).sum() == Q * max(0, k - sum(sizes))
    # every shard full: the same bits as merge_topk on the concatenated lists with global indices
    sizes = [k + r for r in range(world)]
    packed, offsets, lists = packed_shards(sizes, k, Q, 11 * world + k)
    v, i = rank.merge_packed_topk(packed, dev(offsets), k)
    want_v, want_i = R.unpack_merge(host(packed), offsets, k)
    R.assert_selection_equal(host(v), host(i), want_v, want_i, f"packed, full shards world={world} k={k}")
    cat_v = np.concatenate([lv for lv, _ in lists], 1)
    cat_i = np.concatenate([li + off for (_, li), off in zip(lists, offsets)], 1)
    mv, mi = M.merge_topk(dev(cat_v), dev(cat_i), k)
    assert torch.equal(mi, i) and torch.equal(mv.view(torch.int32), v.view(torch.int32))


# ---- k_hit_counts (256 threads per block) and k_distinct_topn (128)
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 129, 257])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 40])
def test_hit_counts_and_distinct_classes_on_mixed_lists(Q, k):
    G = 50
    rng = np.random.default_rng(Q * 100 + k)
    gcls = rng.integers(0, 6, G).astype(np.int64) + 2 ** 33           # few classes: lists with fewer than n distinct ones
    qcls = rng.integers(0, 6, Q).astype(np.int64) + 2 ** 33
    idx = rng.integers(0, G, (Q, k)).astype(np.int64)
    pads = np.array([-1, G, R.IDX_PAD, 2 ** 62], np.int64)
    for j in range(k):                                                # pads at positions 0, 1, 2 and later, interleaved
        rows = np.flatnonzero((np.arange(Q) + j) % 3 == 0)
        idx[rows, j] = pads[(rows + j) % 4]
    if Q > 2:
        idx[2, :] = R.IDX_PAD                                         # an all-pad list
    val = rng.standard_normal((Q, k)).astype(np.float32)
    got = M.hit_counts(dev(idx), dev(qcls), dev(gcls))
    assert tuple(host(got).tolist()) == R.hit_counts(idx, qcls, gcls)
    for n in (1, 3, 8):
        oc, oi, ov = M.distinct_class_topn(dev(idx), dev(val), dev(gcls), n)
        want_c, want_i, want_v = R.distinct_topn(idx, val, gcls, n)
        np.testing.assert_array_equal(host(oc), want_c)
        np.testing.assert_array_equal(host(oi), want_i)
        np.testing.assert_array_equal(R.bits(host(ov))[want_i >= 0], R.bits(want_v)[want_i >= 0])
        assert np.isnan(host(ov)[want_i < 0]).all()
