"""Inputs and exact references for the tests of the cosine GEMM's two-launch tile split (tests/test_rank_tiles_gpu.py,
tests/test_rank_tiles_args.py), in numpy.

LATTICE ROWS.  Every query and gallery row has exactly 16 non-zero entries at random positions, +-0.25 (a unit row: 16 / 16 = 1)
or +-1 (a raw row of norm 4, for ``gallery_is_normalized = 0``; 1 / 4 and x * 0.25 are exact).  A score is then (the signed
overlap of two rows) / 16, an integer multiple of 1 / 16 in [-1, 1]: exact in fp32, in the ``h`` plane of the bf16 split (the
other planes are zero), in fp16, and in any summation order.  Every loop family must therefore return the float64 reference bit
for bit, and everything downstream - the order with its many ties, pads, bin counts, CSR hits, ranks, the nearest centroid - is
an integer or an index that numpy computes from the integer overlaps ``S`` (score = S / 16).  No tolerance appears here.

THE SPLIT.  ``round_split`` / ``tile_of`` / ``launches`` restate ``whole_round_tiles``, ``rank_tile_of`` and ``launch_tiles``
(csrc/rank_common.h); ``workgroups`` lists the tile of every workgroup of a GEMM call, optionally with one modelled bug, and
``run_model`` plays an epilogue over those tiles on the CPU, starting from poisoned outputs as the GPU tests do."""
import functools

import numpy as np

BN = 128
NNZ = 16
PAD32 = 2 ** 31 - 1
ANY, SAME, DIFFERENT = 0, 1, 2

# (slots, Q, G) of the GPU matrix; CLASSES below names what each one reaches
CASES = [(6, 100, 9 * 128 - 5), (8, 130, 13 * 128 - 5), (20, 300, 23 * 128 - 28), (8, 128, 15 * 128), (10, 100, 18 * 128 - 5),
         (12, 65, 23 * 128 - 100), (7, 200, 5 * 128 - 1), (40, 300, 25 * 128 - 28)]
# searches of several query blocks (the query_block argument of ranks / nearest): (slots, Q, G, query_block)
BLOCK_CASES = [(20, 300, 23 * 128 - 28, 150), (7, 230, 9 * 128 - 5, 100)]
EPILOGUES = ["slab", "topk1", "topk2", "topk3", "topk8", "filt1", "filt2", "filt3", "filt8", "topk9", "roc", "range", "ranks",
             "nearest"]
BUGS = ["tail_from_column_0", "tail_with_main_ny", "table_without_x0", "seam_tie_to_higher_index", "tail_tile_twice"]


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the split, restated
def round_split(ntx, ny, slots):
    """``whole_round_tiles``: the column tiles of the main launch."""
    n = ntx * ny
    if n > slots and n % slots != 0:
        return (n // slots) * slots // ny
    return ntx


def tile_of(L, ntiles, ny):
    """``rank_tile_of``: workgroup L of a launch over ntiles column tiles x ny query tiles -> (tx, ty)."""
    full = (ntiles >> 3) << 3
    if L < full * ny:
        g, r = divmod(L, 8 * ny)
        return g * 8 + (r & 7), r >> 3
    r, rem = L - full * ny, ntiles - full
    ty = r // rem
    return full + r - ty * rem, ty


def launches(Q, G, slots):
    """``launch_tiles`` for one GEMM call: [(MT, x0, xtiles, ny)].  slots = 0: a device with room for every tile."""
    ntx = cdiv(G, BN)
    if Q <= 64:
        return [(1, 0, ntx, cdiv(Q, 64))]
    ny = cdiv(Q, 128)
    x1 = round_split(ntx, ny, slots) if slots else ntx
    out = [(2, 0, x1, ny)] if x1 > 0 else []
    if x1 < ntx:
        out.append((1, x1, ntx - x1, cdiv(Q, 64)))
    return out


def report(Q, G, slots):
    """What ``mi355_rank_last_tiles`` reports after that call, without out[0] (the slots)."""
    ntx = cdiv(G, BN)
    if Q <= 64:
        return (cdiv(Q, 64), ntx, 0, 0)
    ny = cdiv(Q, 128)
    x1 = round_split(ntx, ny, slots)
    return (ny, x1, ntx - x1, cdiv(Q, 64) if x1 < ntx else 0)


def seam(Q, G, slots):
    """First gallery row of the tail launch."""
    return round_split(cdiv(G, BN), cdiv(Q, 128), slots) * BN


def blocks(Q, qblock=0):
    qb = qblock if qblock else Q
    return [(q0, min(qb, Q - q0)) for q0 in range(0, Q, qb)]


def workgroups(Q, G, slots, bug=None):
    """The tile of every workgroup of one GEMM call: (m0, m1, n0, n1, table column).  An empty tile (m0 >= Q) is dropped as the
    kernels drop it.  bug: one of BUGS, modelled in the launcher / kernel prologue (the epilogue bugs live in run_model)."""
    out = []
    for MT, x0, xt, ny in launches(Q, G, slots):
        tail = MT == 1 and Q > 64
        ny_used = cdiv(Q, 128) if (tail and bug == "tail_with_main_ny") else ny
        grid = list(range(xt * ny_used))
        if tail and bug == "tail_tile_twice":
            grid.append(grid[0])
        for L in grid:
            tx, ty = tile_of(L, xt, ny_used)
            assert 0 <= tx < xt and 0 <= ty < ny_used
            bx = tx if (tail and bug == "tail_from_column_0") else x0 + tx
            m0, n0 = ty * 64 * MT, bx * BN
            if m0 >= Q:
                continue
            col = tx if (tail and bug == "table_without_x0") else bx
            out.append((m0, min(m0 + 64 * MT, Q), n0, min(n0 + BN, G), col))
    return out


def classes(cases):
    """The split classes a list of (slots, Q, G) reaches, as a set of names."""
    got = set()

    def size(n, who):
        if n < 8:
            return who + "<8"
        return who + ("=8" if n == 8 else ">8+rem" if n % 8 else ">8")

    for slots, Q, G in cases:
        ny, main, tail, tny = report(Q, G, slots)
        if not tail:
            continue
        got |= {size(main, "main"), size(tail, "tail"), "ny=%d" % ny}
        if G % BN:
            got.add("ragged column tile in the tail")
        if Q % 64:
            got.add("ragged query tile in the tail")
    return got


CLASSES = {"main<8", "main=8", "main>8+rem", "tail<8", "tail=8", "tail>8+rem", "ny=1", "ny=2", "ny=3",
           "ragged column tile in the tail", "ragged query tile in the tail"}


# ---------------------------------------------------------------- inputs
def lattice(n, D, rng):
    """n rows of D int8 entries with exactly NNZ non-zeros, each +-1."""
    x = np.zeros((n, D), np.int8)
    pos = np.argsort(rng.random((n, D)), axis=1)[:, :NNZ]
    x[np.arange(n)[:, None], pos] = rng.choice(np.array([-1, 1], np.int8), (n, NNZ))
    return x


class Data:
    """One case's inputs: integer rows (x 0.25: unit rows; x 1: raw rows), labels, exclude, idx_offset, thresholds, and the
    integer overlaps S (score = S / 16)."""

    def __init__(self, Q, G, D, seed, seam_row=None, mode=SAME):
        rng = np.random.default_rng(seed)
        self.Q, self.G, self.D, self.mode, self.cache = Q, G, D, mode, {}
        self.qi, self.gi = lattice(Q, D, rng), lattice(G, D, rng)
        self.off = int(rng.integers(1, 5000))
        self.ql = rng.integers(0, 5, Q).astype(np.int64)
        self.gl = rng.integers(0, 5, G).astype(np.int64)
        self.excl = (rng.integers(0, G, Q) + self.off).astype(np.int64)
        self.excl[rng.random(Q) < 0.3] = -1
        if seam_row is not None and 0 < seam_row < G:
            # ties across the seam: queries 0..3 are bit copies of one row on either side of it, eligible under either label mode
            # (0, 1: the query's label; 2, 3: another one); the last two queries have 0 and 2 rows of their label (pads)
            lo = rng.choice(seam_row, 5, replace=False)
            hi = seam_row + rng.choice(G - seam_row, 5, replace=False)
            for p in range(4):
                self.gi[lo[p]] = self.gi[hi[p]] = self.qi[p]
                self.gl[lo[p]] = self.gl[hi[p]] = self.ql[p] if p < 2 else self.ql[p] + 7
                self.excl[p] = -1
            self.ql[Q - 1], self.ql[Q - 2] = 777, 888
            self.gl[lo[4]] = self.gl[hi[4]] = 888
            self.gi[lo[4]] = self.gi[hi[4]] = self.qi[Q - 1]         # the last query row is the nearest of a column on either side
            self.excl[Q - 2] = -1
        self.S = np.rint(self.qi.astype(np.float64) @ self.gi.astype(np.float64).T).astype(np.int32)   # (exact: small integers)
        assert np.abs(self.S).max() <= NNZ
        # thresholds on lattice values (the >= boundary) and between them; the ROC grid has duplicates
        self.t_on, self.t_between = 3 / 16, 3.5 / 16
        grid = np.concatenate([rng.choice(np.arange(-4, 7), 4) / 16, (rng.choice(np.arange(-4, 7), 4) + 0.5) / 16, [1.0]])
        self.thr = np.sort(np.concatenate([grid, grid[[0, 5]]])).astype(np.float64)

    def rows(self, which, raw):
        x = self.qi if which == "q" else self.gi
        return x.astype(np.float32) * np.float32(1.0 if raw else 0.25)

    def eligible(self, mode, use_excl=True):
        ok = np.ones((self.Q, self.G), bool)
        if mode == SAME:
            ok &= self.ql[:, None] == self.gl[None, :]
        elif mode == DIFFERENT:
            ok &= self.ql[:, None] != self.gl[None, :]
        if use_excl:
            ok &= (np.arange(self.G)[None, :] + self.off) != self.excl[:, None]
        return ok


@functools.lru_cache(maxsize=64)
def case_data(slots, Q, G, D, qblock=0):
    i = CASES.index((slots, Q, G)) if (slots, Q, G) in CASES else len(CASES) + BLOCK_CASES.index((slots, Q, G, qblock))
    q_call = blocks(Q, qblock)[0][1]
    return Data(Q, G, D, 1000 * i + D, seam(q_call, G, slots), [SAME, DIFFERENT, ANY][i % 3])


def f32(S):
    """The fp32 score of integer overlaps."""
    return (np.asarray(S, np.float64) / 16).astype(np.float32)


def score_keys(s):
    """``score_key`` (csrc/rank_common.h) of finite fp32 scores."""
    u = (np.asarray(s, np.float32) + np.float32(0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# ---------------------------------------------------------------- references (from S, in one piece)
def _select(vals, idx, k, seam_row=None):
    """Top-k of each row of candidates: vals float64 (NaN first, as the kernels order it; -inf = pad), idx int64.  Order: higher
    value, then lower index.  seam_row (a modelled bug): among equal values an index at or past the seam goes first."""
    rank = np.where(np.isnan(vals), -1000, np.where(np.isneginf(vals), 1000, np.rint(-16 * np.where(np.isfinite(vals), vals, 0))))
    tie = idx.astype(np.int64)
    if seam_row is not None:
        tie = np.where(tie >= seam_row, tie - (1 << 40), tie)
    comp = (rank.astype(np.int64) + 1000) * (1 << 42) + (tie + (1 << 41))
    if k < comp.shape[1]:
        part = np.argpartition(comp, k - 1, axis=1)[:, :k]
    else:
        part = np.broadcast_to(np.arange(comp.shape[1]), comp.shape)
    r = np.arange(vals.shape[0])[:, None]
    order = part[r, np.argsort(comp[r, part], axis=1)][:, :k]
    return vals[r, order], idx[r, order]


def _finish_topk(v, i, off):
    pad = np.isneginf(v)
    return np.where(pad, -np.inf, v).astype(np.float32), np.where(pad, -1, i + off).astype(np.int64)


def topk_ref(d, k, elig=None, seam_row=None):
    """(values fp32 [Q][k], indices int64 [Q][k]): descending, ties to the lower index, (-inf, -1) pads under a filter."""
    vals = d.S.astype(np.float64) / 16
    if elig is not None:
        vals = np.where(elig, vals, -np.inf)
    idx = np.broadcast_to(np.arange(d.G, dtype=np.int64), vals.shape)
    return _finish_topk(*_select(vals, idx, k, seam_row), d.off)


def roc_ref(d):
    """hist int64 [2][T + 1]: genuine / impostor pairs whose score is >= exactly b thresholds (float64), exclusions left out."""
    b = np.searchsorted(d.thr, d.S.astype(np.float64) / 16, side="right")
    ok = d.eligible(ANY)
    same = d.ql[:, None] == d.gl[None, :]
    T = d.thr.shape[0]
    return np.stack([np.bincount(b[ok & same], minlength=T + 1), np.bincount(b[ok & ~same], minlength=T + 1)]).astype(np.int64)


def range_ref(d, t, elig):
    """(offsets [Q + 1], indices, scores): the eligible pairs with score >= t in float64, rows ascending per query."""
    hit = (d.S.astype(np.float64) / 16 >= t) & elig
    qi, gi = np.nonzero(hit)
    offsets = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.int64)
    return offsets, (gi + d.off).astype(np.int64), f32(d.S[qi, gi])


def ranks_ref(d):
    """``_ranks_ref``, computed once per Data."""
    if "ranks" not in d.cache:
        d.cache["ranks"] = _ranks_ref(d)
    return d.cache["ranks"]


def _ranks_ref(d):
    """The four steps of the full-gallery ranks: the positives as CSR (row order), their composites, rank order, ``before``, the
    ranks, AP and first rank."""
    ok = d.eligible(ANY)
    pos = ok & (d.ql[:, None] == d.gl[None, :])
    keys = score_keys(f32(d.S)).astype(np.uint64)
    comp = (keys << np.uint64(32)) | (~np.arange(d.G, dtype=np.uint32)).astype(np.uint64)[None, :]
    offsets = np.concatenate([[0], np.cumsum(pos.sum(1))]).astype(np.int64)
    out = dict(offsets=offsets, row_indices=(np.nonzero(pos)[1] + d.off).astype(np.int64), row_scores=f32(d.S[pos]),
               row_keys=comp[pos])
    n = int(offsets[-1])
    sk, si, before, ranks = (np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.uint32), np.zeros(n, np.int64))
    ap, first = np.zeros(d.Q, np.float64), np.zeros(d.Q, np.int64)
    for q in range(d.Q):
        s0, s1 = offsets[q], offsets[q + 1]
        R = s1 - s0
        if R == 0:
            continue
        cols = np.nonzero(pos[q])[0]
        order = np.argsort(comp[q, cols])[::-1]                  # composites are distinct: descending = rank order
        sk[s0:s1], si[s0:s1] = comp[q, cols][order], cols[order] + d.off
        neg = comp[q, ok[q] & ~pos[q]]
        asc = sk[s0:s1][::-1].copy()
        beat = R - np.searchsorted(asc, neg, side="right")       # positives whose composite is above the negative's
        before[s0:s1] = np.bincount(beat[beat < R], minlength=R)[:R]
        ranks[s0:s1] = np.arange(1, R + 1) + np.cumsum(before[s0:s1].astype(np.int64))
        # (sum_i (i + 1) / rank_i) / R in float64, the terms added in the order i = 0, 1, .. (cumsum adds one by one)
        ap[q] = np.cumsum(np.arange(1, R + 1, dtype=np.float64) / ranks[s0:s1].astype(np.float64))[-1] / float(R)
        first[q] = ranks[s0]
    out.update(keys=sk, indices=si, before=before, ranks=ranks, ap=ap, first=first)
    return out


def nearest_ref(d):
    """(assign int64 [G], score fp32 [G]): the query row with the highest score per gallery row, ties to the lower one."""
    a = np.argmax(d.S, axis=0).astype(np.int64)
    return a, f32(d.S[a, np.arange(d.G)])


def reference(d, epi):
    """The result of one epilogue of EPILOGUES as a tuple of arrays (computed once per Data; do not write to it)."""
    if ("ref", epi) not in d.cache:
        d.cache["ref", epi] = _reference(d, epi)
    return d.cache["ref", epi]


def _reference(d, epi):
    if epi == "slab":
        return (f32(d.S),)
    if epi.startswith("topk"):
        return topk_ref(d, int(epi[4:]))
    if epi.startswith("filt"):
        return topk_ref(d, int(epi[4:]), d.eligible(d.mode))
    if epi == "roc":
        return (roc_ref(d),)
    if epi == "range":
        return range_ref(d, d.t_on, d.eligible(d.mode)) + range_ref(d, d.t_between, d.eligible(d.mode))
    if epi == "ranks":
        r = ranks_ref(d)
        return tuple(r[k] for k in ("offsets", "row_indices", "row_scores", "row_keys", "before", "ranks", "ap", "first"))
    if epi == "nearest":
        return nearest_ref(d)
    raise ValueError(epi)


def applies(bug, epi):
    """Whether a modelled bug can reach an epilogue: the (query, column tile) tables belong to the fused selection and the range
    pass (the ranks read their positives from it); the tie rule to the selections; only accumulating epilogues see a tile that
    runs twice (a slab, a candidate list and a maximum are idempotent)."""
    if bug == "table_without_x0":
        return (epi[:4] in ("topk", "filt") and int(epi[4:]) <= 8) or epi in ("range", "ranks")
    if bug == "seam_tie_to_higher_index":
        return epi[:4] in ("topk", "filt")
    if bug == "tail_tile_twice":
        return epi in ("roc", "range", "ranks")
    return True


# ---------------------------------------------------------------- the epilogues, tile by tile
def _model_range(d, wgs, t, elig, ntx):
    """The range epilogue and its compaction: per tile the hits of each row, one reservation per tile, a (query, tile) table
    walked in tile order.  A table cell no tile wrote is poison (one hit at row -1).  Returns the CSR and the hit counter."""
    hit = elig & ((d.S.astype(np.float64) / 16 >= t) if t is not None else True)
    cell = np.zeros((d.Q, ntx, BN), bool)
    src = np.full((d.Q, ntx, BN), -1, np.int64)
    cell[:, :, 0] = True                                              # poison until a tile writes the cell
    cursor = 0
    for m0, m1, n0, n1, col in wgs:
        cell[m0:m1, col] = False
        cell[m0:m1, col, : n1 - n0] = hit[m0:m1, n0:n1]
        src[m0:m1, col, : n1 - n0] = np.arange(n0, n1)
        cursor += int(hit[m0:m1, n0:n1].sum())
    cell, src = cell.reshape(d.Q, -1), src.reshape(d.Q, -1)
    qi, pi = np.nonzero(cell)
    gi = src[qi, pi]
    offsets = np.concatenate([[0], np.cumsum(cell.sum(1))]).astype(np.int64)
    return offsets, gi + d.off, f32(np.where(gi >= 0, d.S[qi, np.maximum(gi, 0)], -99)), cursor


def run_model(d, epi, slots, bug=None, qblock=0):
    """One epilogue played tile by tile over the workgroups of every GEMM call of the search, from poisoned outputs (NaN scores,
    -1 indices: what 0xFF bytes read as), with at most one modelled bug.  Without a bug it must equal ``reference``."""
    Q, G, ntx = d.Q, d.G, cdiv(d.G, BN)
    sc = d.S.astype(np.float64) / 16
    calls = [(q0, workgroups(qn, G, slots, bug)) for q0, qn in blocks(Q, qblock)]
    wgs = [(q0 + m0, q0 + m1, n0, n1, col) for q0, w in calls for m0, m1, n0, n1, col in w]
    seam_row = seam(blocks(Q, qblock)[0][1], G, slots) if bug == "seam_tie_to_higher_index" else None
    if epi == "slab" or epi == "topk9":
        out = np.full((Q, G), np.nan)
        for m0, m1, n0, n1, _ in wgs:
            out[m0:m1, n0:n1] = sc[m0:m1, n0:n1]
        if epi == "slab":
            return (out.astype(np.float32),)
        idx = np.broadcast_to(np.arange(G, dtype=np.int64), out.shape)
        return _finish_topk(*_select(out, idx, 9, seam_row), d.off)
    if epi[:4] in ("topk", "filt"):
        k = int(epi[4:])
        elig = d.eligible(d.mode) if epi[:4] == "filt" else np.ones((Q, G), bool)
        cv, ci = np.full((Q, ntx, k), np.nan), np.full((Q, ntx, k), -1, np.int64)
        for m0, m1, n0, n1, col in wgs:
            v = np.where(elig[m0:m1, n0:n1], sc[m0:m1, n0:n1], -np.inf)
            v = np.pad(v, ((0, 0), (0, max(0, k - v.shape[1]))), constant_values=-np.inf)
            i = np.broadcast_to(n0 + np.arange(v.shape[1], dtype=np.int64), v.shape)
            tv, ti = _select(v, i, k)
            cv[m0:m1, col], ci[m0:m1, col] = tv, np.where(np.isneginf(tv), PAD32, ti)
        return _finish_topk(*_select(cv.reshape(Q, -1), ci.reshape(Q, -1), k, seam_row), d.off)
    if epi == "roc":
        T = d.thr.shape[0]
        hist = np.zeros((2, T + 1), np.int64)
        ok, same = d.eligible(ANY), d.ql[:, None] == d.gl[None, :]
        for m0, m1, n0, n1, _ in wgs:
            b = np.searchsorted(d.thr, sc[m0:m1, n0:n1], side="right")
            o, s = ok[m0:m1, n0:n1], same[m0:m1, n0:n1]
            hist[0] += np.bincount(b[o & s], minlength=T + 1)
            hist[1] += np.bincount(b[o & ~s], minlength=T + 1)
        return (hist,)
    if epi == "range":
        a = _model_range(d, wgs, d.t_on, d.eligible(d.mode), ntx)
        b = _model_range(d, wgs, d.t_between, d.eligible(d.mode), ntx)
        ref = reference(d, "range")
        # the hit counter is part of the result: a count that differs from the CSR total is reported as an extra array
        extra = () if (a[3], b[3]) == (int(ref[0][-1]), int(ref[3][-1])) else (np.array([a[3], b[3]]),)
        return a[:3] + b[:3] + extra
    if epi == "ranks":
        ok = d.eligible(ANY)
        pos = ok & (d.ql[:, None] == d.gl[None, :])
        # the positives: the range pass without a threshold, always ONE GEMM call per range query block (the whole Q here)
        offsets, gidx, gsc, _ = _model_range(d, workgroups(Q, G, slots, bug), None, pos, ntx)
        r = ranks_ref(d)
        if not (np.array_equal(offsets, r["offsets"]) and np.array_equal(gidx, r["row_indices"])):
            return (offsets, gidx, gsc)                                  # the counting pass has nothing sound to count into
        keys = score_keys(f32(d.S)).astype(np.uint64)
        comp = (keys << np.uint64(32)) | (~np.arange(G, dtype=np.uint32)).astype(np.uint64)[None, :]
        before = np.zeros_like(r["before"])
        times = np.zeros((Q, G), np.int64)                               # how often a tile counted each pair
        for m0, m1, n0, n1, _ in wgs:
            times[m0:m1, n0:n1] += 1
        for q in range(Q):
            s0, s1 = r["offsets"][q], r["offsets"][q + 1]
            R, neg = s1 - s0, ok[q] & ~pos[q]
            if R == 0:
                continue
            beat = R - np.searchsorted(r["keys"][s0:s1][::-1], comp[q, neg], side="right")
            w = times[q, neg]
            before[s0:s1] = np.bincount(beat[beat < R], weights=w[beat < R], minlength=R)[:R].astype(np.uint32)
        ranks = np.zeros_like(r["ranks"])
        for q in range(Q):
            s0, s1 = r["offsets"][q], r["offsets"][q + 1]
            ranks[s0:s1] = np.arange(1, s1 - s0 + 1) + np.cumsum(before[s0:s1].astype(np.int64))
        # (AP and the first rank are functions of the ranks: a model whose ranks equal the reference's has them too)
        same = np.array_equal(ranks, r["ranks"])
        return (r["offsets"], r["row_indices"], r["row_scores"], r["row_keys"], before, ranks,
                r["ap"] if same else np.zeros_like(r["ap"]), r["first"] if same else np.zeros_like(r["first"]))
    if epi == "nearest":
        best = np.zeros(G, np.uint64)                                    # (zeroed by the host before the first call)
        keys = score_keys(f32(d.S)).astype(np.uint64)
        for m0, m1, n0, n1, _ in wgs:
            k64 = (keys[m0:m1, n0:n1] << np.uint64(32)) | (~np.arange(m0, m1, dtype=np.uint32)).astype(np.uint64)[:, None]
            best[n0:n1] = np.maximum(best[n0:n1], k64.max(axis=0))
        a = (~(best & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64)
        u = (best >> np.uint64(32)).astype(np.uint32)
        s = np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
        return a, s
    raise ValueError(epi)


def same_result(a, b):
    """Tuples of arrays equal element for element (floats by their bits, so that a NaN or a -0 counts as a difference)."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32 if x.itemsize == 4 else np.uint64), y.view(np.uint32 if y.itemsize == 4 else np.uint64)
        if not np.array_equal(x, y):
            return False
    return True
