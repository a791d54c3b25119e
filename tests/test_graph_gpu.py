"""The graph search on the GPU against its NumPy model (tests/graph_ref.py), bit for bit: indices, score bits, the number of
expansions and the size of the visited set.  The model's score matrix comes from ``mi355_rescore_candidates`` over all rows -
the walk is specified on top of those scores - so the galleries are small (at most 600 rows, 2000 for ``build``).  The graphs
are hand-made: the test controls pads, self-loops, duplicates, components and how many unseen rows an expansion finds."""
import functools

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import graph_ref as ref
import stream_harness as H
from helpers import SCORE_TOL
from imageretrievalresearch_amd import _lib, graph
from imageretrievalresearch_amd import rank as _rank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16}
G, NQ = 600, 67
DIMS = [1, 7, 70, 1536]


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _raw(seed, n, D):
    return (np.random.default_rng(seed).standard_normal((n, D)) * 1.3).astype(np.float32)


def scores_of(g, x):
    """(Q, rows) float32 on the host: what mi355_rescore_candidates gives every (query, row) pair - the model's input."""
    Q, n, L = x.shape[0], g.rows, _lib.lib()
    cand = torch.arange(n, dtype=torch.int64, device=DEV).repeat(Q, 1).contiguous()
    out = torch.empty((Q, n), dtype=torch.float32, device=DEV)
    ws = torch.empty(L.mi355_rescore_candidates_workspace_bytes(Q, g.dim), dtype=torch.uint8, device=DEV)
    _lib.check(L.mi355_rescore_candidates(x.data_ptr(), Q, g.dim, g.eps, g._buf.data_ptr(), _rank._DTYPES[g.dtype], g._ld, n,
                                          cand.data_ptr(), n, 0, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(DEV)))
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _setup(kind, D):
    """(gallery of G labelled rows, NQ queries on the device, their scores, gallery labels, query labels): made once."""
    glab = np.random.default_rng(3).integers(0, 4, G)
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(_raw(1, G, D)).to(DEV), labels=torch.from_numpy(glab).to(DEV))
    x = torch.from_numpy(_raw(2, NQ, D)).to(DEV)
    return g, x, scores_of(g, x), glab, np.random.default_rng(4).integers(0, 4, NQ)


def _index(g, adj):
    """An index of hand-made parts: the graph, and one entry point that no test uses (the seeds are given)."""
    return M.GraphIndex(g, torch.from_numpy(np.ascontiguousarray(adj, dtype=np.int32)).to(DEV),
                        torch.zeros(1, dtype=torch.int64, device=DEV), torch.ones((1, g.dim), device=DEV))


# ---- the graphs
def ring(n, R):
    """A ring with chords: row r lists r + 1, r - 1, r + 4, r - 9, r + 16, ... (mod n)."""
    off = [(j // 2 + 1) ** 2 * (1 if j % 2 == 0 else -1) for j in range(R)]
    return np.stack([[(r + o) % n for o in off] for r in range(n)]).astype(np.int32)


def messy(n, R, seed=5):
    """Random lists with pads anywhere, self-loops (every third row) and duplicates within a list (every fourth row)."""
    a = np.random.default_rng(seed + R).integers(-1, n, (n, R)).astype(np.int32)
    a[::3, 0] = np.arange(n)[::3]
    a[::4, R - 1] = a[::4, 1 if R > 2 else 0]
    a[5] = -1                                                    # a row without neighbours
    return a


def two_components(n, R):
    """Two rings with chords that never meet: rows [0, n / 2) and [n / 2, n)."""
    h = n // 2
    half = ring(h, R)
    return np.concatenate([half, half + h]).astype(np.int32)


def complete(n):
    return np.stack([[j for j in range(n) if j != r] for r in range(n)]).astype(np.int32)


def _seeds(Q, nseed, hi, seed=0):
    """Random rows below ``hi``, with skipped slots (-1) and repeats; every query keeps at least one real seed."""
    s = np.random.default_rng(1000 * Q + nseed + seed).integers(-1, hi, (Q, nseed)).astype(np.int64)
    s[:, 0] = np.abs(s[:, 0])
    if nseed > 2:
        s[:, 2] = s[:, 0]
    return s


def _run(ix, x, seeds, k, ef, max_iters=None, **kw):
    v, i, it, vis = ix.search(x, k, ef, seeds=torch.from_numpy(seeds).to(DEV), max_iters=max_iters, stats=True, **kw)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and it.dtype == torch.int32 and vis.dtype == torch.int32
    assert tuple(v.shape) == tuple(i.shape) == (x.shape[0], k) and tuple(it.shape) == tuple(vis.shape) == (x.shape[0],)
    return v.cpu().numpy(), i.cpu().numpy(), it.cpu().numpy(), vis.cpu().numpy()


def _same(got, want, what):
    for name, a, b in zip(("values", "indices", "iters", "visited"), got, want):
        bad = np.nonzero((_bits(a) != _bits(b)).reshape(a.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differ for queries {bad[:8].tolist()}: {a[bad[0]]} != {b[bad[0]]}"


# (graph, R, Q, k, ef, nseed, max_iters): every value of Q {1, 3, 5, 67}, k {1, 3, 8, 64}, ef {k, 2, 63, 64, 65, 512},
# R {2, 6, 8, 32, 64}, nseed {1, 8, 64} and max_iters {1, 3, default} occurs, the extremes together
CONFIGS = [
    (ring, 2, 1, 1, 1, 1, None),
    (ring, 6, 3, 3, 3, 8, 3),
    (ring, 8, 67, 8, 63, 8, None),
    (ring, 32, 5, 64, 64, 64, None),
    (ring, 64, 3, 3, 65, 8, 1),
    (ring, 2, 1, 64, 512, 8, None),                              # 600 expansions: the walk covers the ring
    (messy, 6, 67, 1, 2, 8, None),
    (messy, 8, 5, 8, 64, 1, None),
    (messy, 32, 3, 64, 512, 64, 3),
    (messy, 64, 5, 3, 65, 8, None),
    (messy, 64, 1, 64, 512, 64, None),                           # the largest beam, list and seed count at once
    (two_components, 6, 5, 64, 512, 8, None),
]


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kind", list(DTYPES))
def test_hand_made_graphs_match_the_model(kind, D):
    g, x, S, _, _ = _setup(kind, D)
    for make, R, Q, k, ef, nseed, max_iters in CONFIGS:
        adj = make(G, R)
        ix = _index(g, adj)
        seeds = _seeds(Q, nseed, G // 2 if make is two_components else G)
        mi = ix.default_max_iters(ef, nseed) if max_iters is None else max_iters
        got = _run(ix, x[:Q], seeds, k, ef, max_iters)
        want = ref.search(S[:Q], adj, seeds, k, ef, mi)
        what = f"{kind} D={D} {make.__name__} R={R} Q={Q} k={k} ef={ef} nseed={nseed} max_iters={max_iters}"
        _same(got, want, what)
        assert (got[2] <= mi).all() and (got[3] <= nseed + got[2] * R).all() and (got[2] >= 1).all(), what
        if make is two_components:                               # the seeds lie in the first ring: the second is never reached
            assert (got[1] < G // 2).all() and (got[3] <= G // 2).all(), what
        if max_iters == 1:
            assert (got[2] == 1).all(), what


@pytest.mark.parametrize("kind", list(DTYPES))
def test_tree_every_expansion_finds_R_unseen_rows(kind):
    """Rows on a quarter circle whose score against the query falls with the row id, and a forest whose roots are the seeds
    and whose node r has the children nseed + r * R + j: the walk expands 0, 1, 2, ... and every list is R rows never seen
    before, so the visited set holds exactly nseed + iters * R rows."""
    D = 7
    theta = np.pi / 4 + np.arange(G) * (np.pi / 2) / G
    rows = np.zeros((G, D), np.float32)
    rows[:, 0], rows[:, 1] = np.cos(theta), np.sin(theta)
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(rows).to(DEV))
    x = torch.zeros((3, D), device=DEV)
    x[:, 0] = torch.tensor([1.0, 2.0, 0.5])
    S = scores_of(g, x)
    assert (np.diff(S, axis=1) <= 0).all()                       # the lower row is never the worse one
    for R, nseed, ef, max_iters in ((8, 8, 8, None), (8, 8, 64, None), (64, 8, 2, 3), (6, 1, 63, 1), (32, 1, 3, None), (2, 64, 65, None)):
        adj = np.array([[nseed + r * R + j if nseed + r * R + j < G else -1 for j in range(R)] for r in range(G)], np.int32)
        ix = _index(g, adj)
        seeds = np.tile(np.arange(nseed, dtype=np.int64), (3, 1))
        mi = ix.default_max_iters(ef, nseed) if max_iters is None else max_iters
        got = _run(ix, x, seeds, min(ef, 3), ef, max_iters)
        _same(got, ref.search(S, adj, seeds, min(ef, 3), ef, mi), f"tree {kind} R={R} nseed={nseed} ef={ef}")
        iters = min(mi, ef)                                      # the ef lowest rows are expanded in order, then nothing is left
        assert nseed + iters * R <= G
        assert (got[2] == iters).all() and (got[3] == nseed + iters * R).all(), (R, nseed, ef, got[2], got[3])
        assert (got[1] == np.arange(min(ef, 3))).all()


@pytest.mark.parametrize("kind", list(DTYPES))
def test_complete_graph_with_the_widest_beam_is_the_exhaustive_search(kind):
    n, D = 65, 70
    lab = torch.arange(n, device=DEV) % 3
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(_raw(21, n, D)).to(DEV), labels=lab)
    x = torch.from_numpy(_raw(22, 5, D)).to(DEV)
    S, adj = scores_of(g, x), complete(n)
    ix = _index(g, adj)
    seeds = _seeds(5, 8, n)
    for k in (1, 3, 8, 64):
        got = _run(ix, x, seeds, k, 512)
        _same(got, ref.search(S, adj, seeds, k, 512, ix.default_max_iters(512, 8)), f"complete {kind} k={k}")
        assert (got[2] == n).all() and (got[3] == n).all()
        ev, ei = g.search(x, k)
        assert (got[1] == ei.cpu().numpy()).all() and np.abs(got[0] - ev.cpu().numpy()).max() <= SCORE_TOL
    # fewer eligible rows than k: the same pads as the exhaustive search
    ql = torch.tensor([0, 1, 2, 0, 1], device=DEV)
    v, i = ix.search(x, 64, 512, seeds=torch.from_numpy(seeds).to(DEV), query_labels=ql, label_filter="same")
    ev, ei = g.search(x, 64, query_labels=ql, label_filter="same")
    assert (i == ei).all() and (i == -1).any() and (torch.isneginf(v) == torch.isneginf(ev)).all()
    fin = ~torch.isneginf(ev)
    assert (v[fin] - ev[fin]).abs().max().item() <= SCORE_TOL and (i[~fin] == -1).all()


@pytest.mark.parametrize("kind", list(DTYPES))
def test_filters_choose_among_the_beam_and_leave_the_walk_alone(kind):
    g, x, S, glab, qlab = _setup(kind, 70)
    adj, Q, k, ef = messy(G, 8), 67, 8, 65
    ix = _index(g, adj)
    seeds = _seeds(Q, 8, G)
    mi = ix.default_max_iters(ef, 8)
    plain = _run(ix, x, seeds, k, ef)
    ql = torch.from_numpy(qlab).to(DEV)
    ex = plain[1][:, 0].copy() + 1000                            # every query's best row, as a global index
    ex[::5] = -1
    for label_filter in (None, "same", "different"):
        for exclude in (None, ex):
            if label_filter is None and exclude is None:
                continue
            kw = dict(label_filter=label_filter, idx_offset=1000)
            if label_filter is not None:
                kw["query_labels"] = ql
            if exclude is not None:
                kw["exclude"] = torch.from_numpy(exclude).to(DEV)
            got = _run(ix, x, seeds, k, ef, **kw)
            el = ref.eligible_mask(Q, G, qlab, glab, label_filter, exclude, idx_offset=1000)
            _same(got, ref.search(S, adj, seeds, k, ef, mi, el, idx_offset=1000), f"{kind} {label_filter} {exclude is not None}")
            assert (got[2] == plain[2]).all() and (got[3] == plain[3]).all()       # the counters do not see the filter
            if exclude is not None:
                assert (got[1][exclude >= 0] != exclude[exclude >= 0, None]).all()
    off = _run(ix, x, seeds, k, ef, idx_offset=1000)
    assert (off[1] == plain[1] + 1000).all() and (_bits(off[0]) == _bits(plain[0])).all()


@pytest.mark.parametrize("kind", list(DTYPES))
def test_a_query_does_not_depend_on_its_batch_and_runs_repeat(kind):
    g, x, S, _, _ = _setup(kind, 1536)
    adj = ring(G, 8)
    ix = _index(g, adj)
    seeds = _seeds(NQ, 8, G)
    whole = _run(ix, x, seeds, 8, 64)
    _same(_run(ix, x, seeds, 8, 64), whole, "a second run")
    for q in range(NQ):
        one = _run(ix, x[q: q + 1], seeds[q: q + 1], 8, 64)
        _same(one, tuple(a[q: q + 1] for a in whole), f"query {q} alone")
    # the queries in another order, beside other queries
    perm = np.random.default_rng(9).permutation(NQ)
    _same(_run(ix, x[torch.from_numpy(perm).to(DEV)], seeds[perm], 8, 64), tuple(a[perm] for a in whole), "permuted")


# ---- the limits the header declares, the visited set's wrap, and the beam's order among equal and NaN scores
@pytest.mark.parametrize("kind", list(DTYPES))
def test_the_largest_launch(kind):
    """dim 4096, ef 512 and nseed + max_iters * degree = 16384 together: the dynamic LDS the launcher declares as its maximum
    (the query, two beams, the hop's rows and a 32768-slot visited set: 156,176 bytes)."""
    D, R, nseed, ef, max_iters, Q, k = graph.MAX_DIM, graph.MAX_DEGREE, graph.MAX_NSEED, graph.MAX_EF, 255, 3, 64
    assert (D, R, nseed, ef) == (4096, 64, 64, 512) and nseed + max_iters * R == graph.MAX_VISITS == 16384
    slots = 8
    while slots < 2 * (nseed + max_iters * R):
        slots *= 2
    assert slots == 32768 and 4 * D + 2 * ef * 8 + 2 * 64 * 4 + 16 + 4 * slots == 156176
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(_raw(1, G, D)).to(DEV))
    x = torch.from_numpy(_raw(2, Q, D)).to(DEV)
    S, adj = scores_of(g, x), messy(G, R)
    ix = _index(g, adj)
    seeds = _seeds(Q, nseed, G)
    got = _run(ix, x, seeds, k, ef, max_iters)
    _same(got, ref.search(S, adj, seeds, k, ef, max_iters), f"largest launch {kind}")
    assert (got[2] == max_iters).all() and (got[3] > ef).all()      # the walk ran to its last hop with a full beam


def _slot_of(row, slots):
    """Where the visited set's probe of ``row`` begins - restated from graph.hip: the top log2(slots) bits of the 32-bit
    product row * 2654435761."""
    return ((int(row) * 2654435761) & 0xffffffff) >> (32 - (slots.bit_length() - 1))


@pytest.mark.parametrize("nseed,R,max_iters,slots", [(1, 2, 1, 8), (2, 2, 3, 16), (8, 8, 3, 64)])
def test_the_visited_set_wraps_from_its_last_slot(nseed, R, max_iters, slots):
    """Every row a walk can meet begins its probe at the last slot of the smallest tables (the power of two at or above
    2 * (nseed + max_iters * degree)), so every row but the first goes on to slot 0, 1, ..."""
    table = 8
    while table < 2 * (nseed + max_iters * R):
        table *= 2
    assert table == slots
    g, x, S, _, _ = _setup("f32", 7)
    last = [r for r in range(G) if _slot_of(r, slots) == slots - 1]
    assert len(last) >= max(4, nseed + 1), (slots, last)
    # row r lists the next R rows of `last` (cyclically) after its own place, or after r mod len(last) for the other rows
    place = {r: i for i, r in enumerate(last)}
    adj = np.array([[last[(place.get(r, r) + 1 + j) % len(last)] for j in range(R)] for r in range(G)], np.int32)
    seeds = np.array([[last[(q + j) % len(last)] for j in range(nseed)] for q in range(3)], np.int64)
    assert all(_slot_of(r, slots) == slots - 1 for r in adj[last].reshape(-1)) and all(_slot_of(r, slots) == slots - 1 for r in seeds.reshape(-1))
    ix = _index(g, adj)
    got = _run(ix, x[:3], seeds, 1, min(8, nseed + R), max_iters)
    want = ref.search(S[:3], adj, seeds, 1, min(8, nseed + R), max_iters)
    _same(got, want, f"wrap slots={slots}")
    # at least three distinct rows began at the last slot, so at least two went on to slot 0: none was lost or met twice
    assert (got[3] >= 3).all() and (got[3] >= nseed).all() and (got[3] <= min(len(last), nseed + max_iters * R)).all()
    if slots == 8:                                                   # the seed and its two neighbours, nothing else
        assert (got[2] == 1).all() and (got[3] == 3).all()
    if slots == 64:                                                  # eight seeds and the one row of `last` that is left
        assert (got[3] == len(last)).all() and len(last) == nseed + 1


@pytest.mark.parametrize("kind", list(DTYPES))
def test_equal_zero_and_nan_scores_keep_the_beam_order(kind):
    """Rows r and r + 300 are copies (equal score bits), four rows (and their copies) are zero and five are one-hot (exact zeros
    against a one-hot query), one row is NaN; a query that is a gallery row, a one-hot query and a zero query (every score 0
    or NaN).  The rank-by-count merge gives two entries the same place unless the order is strict on what it meets."""
    D, half = 70, G // 2
    base = _raw(31, half, D).copy()
    base[10:14] = 0.0
    base[30:35] = np.eye(D, dtype=np.float32)[:5]
    rows = np.concatenate([base, base])
    rows[20] = np.nan                                                # (row 320 stays what row 20 was)
    g = M.Gallery(D, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(rows).to(DEV))
    xq = np.stack([rows[5], np.eye(D, dtype=np.float32)[0], np.zeros(D, np.float32), _raw(32, 1, D)[0], rows[315]])
    x = torch.from_numpy(xq).to(DEV)
    Q = x.shape[0]
    S = scores_of(g, x)
    # what the scores hold, before the walk is looked at
    assert np.isnan(S[:, 20]).all() and not np.isnan(np.delete(S, 20, axis=1)).any()
    keep = [r for r in range(half) if r != 20]
    assert (_bits(S[:, keep]) == _bits(S[:, [r + half for r in keep]])).all()
    assert (S[1, 31:35] == 0).all() and (S[1, 10:14] == 0).all() and S[1, 30] > 0.99 and (np.delete(S[2], 20) == 0).all()
    assert S[0, 5] > 0.99 and S[0, 305] == S[0, 5]
    for make in (ring, messy):
        adj = make(G, 8)
        ix = _index(g, adj)
        seeds = _seeds(Q, 8, G)
        seeds[:, 1] = 20                                             # the NaN row is in every beam from the start
        for ef in (2, 63, 64, 512):
            k = min(ef, 64)
            mi = ix.default_max_iters(ef, 8)
            got = _run(ix, x, seeds, k, ef)
            _same(got, ref.search(S, adj, seeds, k, ef, mi), f"order {kind} {make.__name__} ef={ef}")
            assert (got[1][:, 0] == 20).all()                        # NaN first
            for q in range(Q):
                real = got[1][q][got[1][q] >= 0]
                assert len(set(real.tolist())) == real.size, (kind, make.__name__, ef, q)     # no row twice


# ---- build
@functools.lru_cache(maxsize=None)
def _planted():
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((20, 32)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows = (centres[np.repeat(np.arange(20), 100)] + 0.1 * rng.standard_normal((2000, 32))).astype(np.float32)
    qs = (centres[np.arange(100) % 20] + 0.1 * rng.standard_normal((100, 32))).astype(np.float32)
    return rows, qs


@functools.lru_cache(maxsize=None)
def _built(kind):
    rows, _ = _planted()
    g = M.Gallery(32, DEV, dtype=DTYPES[kind]).add(torch.from_numpy(rows).to(DEV), labels=torch.arange(2000, device=DEV) // 100)
    return g, g.graph(64, 16)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_build_and_search_of_planted_clusters(kind):
    g, ix = _built(kind)
    assert isinstance(ix, M.GraphIndex) and ix.degree == 16 and ix.nentry == 64 and ix.rows == 2000 and not ix.stale
    assert ix.graph.dtype == torch.int32 and tuple(ix.graph.shape) == (2000, 16) and ix.graph.is_contiguous()
    assert ix.nbytes == 2000 * 16 * 4 + 64 * 8 + 64 * 32 * 4
    # the graph: the model's merge of the exact 8 nearest neighbours; the entry points: the row nearest every centroid
    fwd = g.knn_graph(8)[1]
    assert (ix.graph.cpu().numpy() == ref.merged_graph(fwd.cpu().numpy(), 16)).all()
    assert (ix.graph[:, :8] == fwd).all() and (ix.graph[:, 8:] >= 0).any() and (ix.graph[:, 8:] == -1).any()
    assert (graph.merged_graph(fwd, 16) == ix.graph).all()
    cent = g.kmeans(64, iters=10, seed=0).centroids
    assert (_bits(ix.centroids) == _bits(cent)).all()
    assert (ix.entries == g.search(cent, 1)[1].reshape(-1)).all()
    # the search: the model on the index's own graph and seeds
    x = torch.from_numpy(_planted()[1]).to(DEV)
    seeds = ix.seeds(x, 8)
    assert (seeds == ix.entries[M.cosine_topk(x, ix.centroids, 8)[1]]).all() and tuple(seeds.shape) == (100, 8)
    S = scores_of(g, x)
    got = tuple(t.cpu().numpy() for t in ix.search(x, 3, 32, 8, stats=True))
    want = ref.search(S, ix.graph.cpu().numpy(), seeds.cpu().numpy(), 3, 32, ix.default_max_iters(32, 8))
    _same(got, want, f"built {kind}")
    v, i = ix.search(x, 3, 32, 8)
    assert (_bits(v) == _bits(got[0])).all() and (i.cpu().numpy() == got[1]).all()
    # a condition on the data and the build, not on the kernel (the GPU equals the model exactly)
    mean, per = ix.recall(x, 3, 32, 8)
    print(f"[graph] {kind}: recall@3 = {mean:.4f} at nseed 8, ef 32; mean iters {got[2].mean():.1f}, visited {got[3].mean():.1f}")
    assert mean >= 0.9 and tuple(per.shape) == (100,)


def test_cache_and_staleness():
    rows, qs = _planted()
    x = torch.from_numpy(rows[:600]).to(DEV)
    g = M.Gallery(32, DEV).add(x)
    a = g.graph(16, 8, iters=2)
    assert g.graph(16, 8, iters=2) is a and g.graph(16, degree=8, iters=2, seed=0) is a
    assert g.graph(16, 8, iters=3) is not a and g.graph(16, 4, iters=2) is not a and g.graph(8, 8, iters=2) is not a
    assert g.graph(16, 8, iters=2, init=x[:16]) is not a                        # a given start is not cached
    q = torch.from_numpy(qs[:5]).to(DEV)
    a.search(q, 3)
    g.add(x[:1])
    assert a.stale
    for call in (lambda: a.search(q, 3), lambda: a.recall(q, 3)):
        with pytest.raises(M.MI355Error, match="stale"):
            call()
    b = g.graph(16, 8, iters=2)
    assert b is not a and b.rows == 601 and not b.stale and g.graph(16, 8, iters=2) is b
    with pytest.raises(M.MI355Error, match="degree"):
        g.graph(16, 7)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_an_id_outside_the_rows_raises_and_is_never_read(kind):
    g, x, S, _, _ = _setup(kind, 7)
    adj = ring(G, 6)
    ix = _index(g, adj)
    good = _seeds(3, 8, G)
    for bad_id in (G, -2, 1 << 40, -(1 << 33)):
        seeds = good.copy()
        seeds[1, 3] = bad_id
        with pytest.raises(M.MI355Error, match="outside"):
            ix.search(x[:3], 3, 16, seeds=torch.from_numpy(seeds).to(DEV))
    for bad_id in (G, -2, (1 << 31) - 1, -(1 << 31)):
        adj2 = adj.copy()
        adj2[:, 4] = bad_id                                      # whichever row is expanded first names it
        with pytest.raises(M.MI355Error, match="outside"):
            _index(g, adj2).search(x[:3], 3, 16, seeds=torch.from_numpy(good).to(DEV))
    # the next call is clean again
    _same(_run(ix, x[:3], good, 3, 16), ref.search(S[:3], adj, good, 3, 16, ix.default_max_iters(16, 8)), "after the errors")


def test_no_query():
    g, x, _, _, _ = _setup("f32", 7)
    ix = _index(g, ring(G, 6))
    v, i, it, vis = ix.search(x[:0], 3, 16, seeds=torch.zeros((0, 4), dtype=torch.int64, device=DEV), stats=True)
    assert tuple(v.shape) == (0, 3) and tuple(i.shape) == (0, 3) and it.numel() == 0 and vis.numel() == 0


# ---- side streams
def _pair(shape):
    return ({"x": torch.from_numpy(_raw(903, *shape)).to(DEV)}, {"x": torch.from_numpy(_raw(904, *shape)).to(DEV)})


def _make_search(dev):
    g, ix = _built("f32")
    ql = torch.arange(37, device=dev) % 20
    return (lambda i: (ix.search(i["x"], 3, 32, 8, stats=True),
                       ix.search(i["x"], 8, 16, 4, query_labels=ql, label_filter="different", idx_offset=7)),) + _pair((37, 32))


def _make_build(dev):
    def op(i):
        ix = M.Gallery(32, dev).add(i["x"]).graph(16, 8, iters=2)
        return ix.graph, ix.entries, ix.centroids
    return (op,) + _pair((700, 32))


STREAM_CASES = [H.Case("GraphIndex.search", ("GraphIndex.search", "GraphIndex.seeds"), _make_search, syncs=True),
                H.Case("GraphIndex.build", ("GraphIndex.build", "Gallery.graph", "merged_graph"), _make_build, syncs=True)]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.name for c in STREAM_CASES])
def test_side_stream_matches_default_stream(case):
    b = H.Built(case, DEV)
    got = b.under_test()
    H.assert_same(got, b.expected, f"{case.name} on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")
