"""The hand-made inputs and the modelled bugs of the re-ranking limit tests (test_rerank_limits_gpu.py on the GPU,
test_rerank_limits_args.py without one): more rows than the scan has threads, sets longer than a wave, weight rows longer than
a workgroup, V'(q) rows on either side of the score kernel's LDS stage, 33 merge sources, and ids that no search returns.
NumPy only.

The constants below are restated from csrc/rerank.hip (the CPU test reads them back from the source): k_kr_scan is one
workgroup of 1024 threads with ceil(R / 1024) rows each; k_kr_sets fills and k_kr_weights sums 64 entries a trip, k_kr_weights
divides 256 a trip; k_kr_score stages V'(q) rows of up to 4096 entries in LDS; k_kr_weights takes dim <= 8192; a set has at most
(32 + 1) (16 + 1) = 561 entries.

Bad ids are -1, G and G + 1 only: the GPU test places every buffer inside a larger allocation whose slack holds poison, so a
broken guard reads or writes memory the test owns."""
import numpy as np

SCAN_THREADS = 1024
WAVE = 64
THREADS = 256
KR_SCORE_LDS = 4096
KR_MAX_DIM = 8192
MAX_K1 = 32
MAX_ROW = (MAX_K1 + 1) * ((MAX_K1 + 1) // 2 + 1)
TOL = 1e-5                                                          # the project's score tolerance (README)
SENTINEL = -7                                                       # what an unwritten output slot keeps


def scan_chunk(R):
    """Rows per thread of k_kr_scan."""
    return (R + SCAN_THREADS - 1) // SCAN_THREADS


def scan_model(counts, bug=None):
    """offsets (R + 1,) as k_kr_scan leaves them, thread by thread.  Bugs: "dropped" - a thread's run loops stop after their
    first row; "doubled" - every later row of a run reads the run's first count again."""
    counts = np.asarray(counts, np.int64)
    R = len(counts)
    chunk = scan_chunk(R)
    out = np.concatenate([[0], counts])                             # a row that no thread writes keeps its count
    runs = []
    for t in range(SCAN_THREADS):
        r0 = min(t * chunk, R)
        r1 = min(r0 + chunk, R)
        runs.append((r0, min(r1, r0 + 1) if bug == "dropped" else r1))
    seen = (lambda r, r0: counts[r0]) if bug == "doubled" else (lambda r, r0: counts[r])
    part = np.array([sum(seen(r, r0) for r in range(r0, r1)) for r0, r1 in runs], np.int64)
    base = np.cumsum(part) - part
    for t, (r0, r1) in enumerate(runs):
        run = base[t]
        for r in range(r0, r1):
            run += seen(r, r0)
            out[r + 1] = run
    return out


def fill_model(entries, bug=None):
    """cols of one row as the rank-counting fill of k_kr_sets writes them from the unsorted set ``entries``, 64 a trip over a
    row pre-filled with SENTINEL.  Bug "dropped": the second and later trips never run."""
    entries = list(entries)
    out = np.full(len(entries), SENTINEL, np.int32)
    for i, x in enumerate(entries):
        if bug == "dropped" and i >= WAVE:
            break
        out[sum(e < x for e in entries)] = x
    return out


# ---- the 193-row graph at k1 = 32 (h = 16) whose R*(0) has 193 entries
G193, K1 = 193, 32
CIRCULANT = (1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 16)
BAD_DUP_ROW = 30


def graph193():
    """Row 0 lists 1 .. 32.  Row c of 1 .. 32 lists its 11 circulant neighbours among 1 .. 32 (reciprocal inside the first 16),
    its own five rows 33 + 5 (c - 1) + i, row 0 at position 16, then 15 other rows of 1 .. 32.  Row r >= 33 lists its owner,
    then the 31 rows after it on the ring 33 .. 192.  R(0) = {0 .. 32}; |R_h(c)| = 17 with 12 members in R(0), and 36 > 34, so
    every candidate brings its five rows: |R*(0)| = 33 + 160."""
    g = np.zeros((G193, K1), np.int64)
    g[0] = np.arange(1, 33)
    for c in range(1, 33):
        circ = [1 + (c - 1 + o) % 32 for o in CIRCULANT]
        own = [33 + 5 * (c - 1) + i for i in range(5)]
        rest = [j for j in range(1, 33) if j != c and j not in circ][:15]
        g[c] = circ + own + [0] + rest
    for r in range(33, G193):
        g[r] = [1 + (r - 33) // 5] + [33 + (r - 33 + 1 + t) % 160 for t in range(31)]
    return g


def query193(equal=None, below=None):
    """The same lists as 193 query rows: every score 0.5 against tau 0.25, so every listed row is a member.  ``equal``: that
    row's tau is 0.5 exactly (still a member); ``below``: that row's tau is the next float32 above 0.5 (no member)."""
    vals = np.full((G193, K1), 0.5, np.float32)
    tau = np.full(G193, 0.25, np.float32)
    if equal is not None:
        tau[equal] = np.float32(0.5)
    if below is not None:
        tau[below] = np.nextafter(np.float32(0.5), np.float32(1))
    return graph193(), vals, tau


def graph193_bad():
    """graph193 with what no search returns, as gallery rows (the lists ARE the graph): a row that lists itself (40), a repeated
    id (41), an all-pad row (42), pads -1, G and G + 1 inside the first h of rows 3, 12 and 20, and in row 30 a repeated id inside
    the first h in the place of a circulant neighbour.  Each of those four rows and its lost partner (5, 11, 21, 14) keeps
    |R_h| = 16 with 11 members in R(0), 33 > 32, so R*(0) loses row 42 only; counted twice, the repeated id would make
    |R_h(30)| = 17, 33 > 34 would fail and R*(0) would lose five rows more."""
    g = graph193()
    g[40, 3] = 40
    g[41, 5] = g[41, 4]
    g[42] = -1
    g[3, 2], g[12, 1], g[20, 0] = -1, G193, G193 + 1
    g[BAD_DUP_ROW, 10] = g[BAD_DUP_ROW, 11]
    return g


def query193_bad():
    """(lists, list_vals, tau) of query rows against graph193_bad(): row 0 starts with -1, G, G + 1; row 1 repeats an id whose
    first occurrence misses tau and whose second would meet it; row 2 is all pads; row 7 lists 7 (a query row is not the
    gallery row of its number, so that is a member like any other)."""
    lists = graph193().copy()
    vals = np.full((G193, K1), 0.5, np.float32)
    tau = np.full(G193, 0.25, np.float32)
    lists[0, :3] = [-1, G193, G193 + 1]
    j = int(lists[1, 4])
    lists[1, 9] = j
    tau[j] = 0.75
    vals[1, 4], vals[1, 9] = 0.5, 1.0
    lists[2] = -1
    lists[7, 0] = 7
    return lists, vals, tau


# ---- rows for the gather-dot
def unit_rows(n, D, seed, classes=8, spread=1.0):
    """(n, D) float32 unit rows around a few centres, so that the dots - and the weights - differ."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((classes, D))[rng.integers(0, classes, n)] + spread * rng.standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


W_G = 640
W_LENGTHS = (64, 0, 1, 65, 256, 257, 600)                          # both sides of a sum trip and of a division trip; an empty row
W_DIMS = (70, 1536, KR_MAX_DIM)


def weight_pattern(bad=False):
    """(offsets int64, cols int32): rows of W_LENGTHS ascending columns over W_G gallery rows.  ``bad``: the rows of 65 and 257
    entries start with -1 and end with G and G + 1 (their lengths stay)."""
    rng = np.random.default_rng(3)
    rows = [np.sort(rng.choice(W_G, n, replace=False)) for n in W_LENGTHS]
    if bad:
        for r in (3, 5):
            rows[r] = np.concatenate([[-1], rows[r][1:-2], [W_G, W_G + 1]])
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return offsets, np.concatenate(rows).astype(np.int32)


def lane_sum32(x):
    """A float32 sum as a wave takes it: lane l adds x[l], x[l + 64], ... in order, then the lanes fold in halves."""
    part = np.zeros(WAVE, np.float32)
    for i, v in enumerate(np.asarray(x, np.float32)):
        part[i % WAVE] += v
    n = WAVE
    while n > 1:
        n //= 2
        part[:n] = part[:n] + part[n:2 * n]
    return part[0]


def weights_model(rows32, gal32, offsets, cols, bug=None):
    """vals float32 of k_kr_weights in plain float32.  Bugs: "sum_trip" - the row sum stops after its first 64 entries;
    "div_trip" - the division stops after its first 256; "pad_is_last" - a column outside [0, G) is read as row G - 1."""
    G = len(gal32)
    out = np.zeros(len(cols), np.float32)
    for r in range(len(offsets) - 1):
        lo, hi = offsets[r], offsets[r + 1]
        if hi == lo:
            continue
        c = cols[lo:hi].astype(np.int64)
        ok = (c >= 0) & (c < G)
        if bug == "pad_is_last":
            c, ok = np.where(ok, c, G - 1), np.ones_like(ok)
        s = gal32[np.where(ok, c, 0)] @ rows32[r]
        e = np.where(ok, np.exp(s - np.float32(1)), np.float32(0)).astype(np.float32)
        tot = lane_sum32(e[:WAVE] if bug == "sum_trip" else e)
        v = e / tot
        if bug == "div_trip":
            v[THREADS:] = e[THREADS:]
        out[lo:hi] = v
    return out


# ---- V'(q) rows on both sides of the score kernel's LDS stage
S_G, S_LAM = 8200, 0.3
S_EXTRA = 4000                                                      # the one column of the 4097-entry row that no gallery row holds
S_HEAVY = (0, 8190, 8192, 8199)                                     # columns that carry a visible share wherever they occur
S_ROWS = {1: 17, 64: 4100, 65: 4101, 300: S_G - 1}                  # entries -> the gallery row that holds them
S_EMPTY = 5                                                         # a gallery row without entries


def _sparse(cols, rng, gain):
    v = rng.uniform(0.5, 1.5, len(cols))
    v[np.isin(cols, S_HEAVY)] *= gain
    return dict(zip((int(c) for c in cols), v / v.sum()))


def score_case():
    """(query rows, gallery rows) as lists of dicts.  Query rows: 4096 entries, the same with column S_EXTRA added (4097), and
    6000 entries.  The 4097-entry row sums to 1 and the 4096-entry row is that row less one entry, value for value, so both take
    the same sums.  Columns 0 and the last one of every query row, and position 4096 of the long ones, are heavy and matched.
    Gallery rows S_ROWS hold 1, 64, 65 and 300 entries (each sums to 1), none holds S_EXTRA."""
    rng = np.random.default_rng(12)
    even = np.arange(0, 8194, 2)
    assert len(even) == KR_SCORE_LDS + 1 and S_EXTRA in even
    b = _sparse(even, rng, 200.0)
    c = {k: v for k, v in b.items() if k != S_EXTRA}
    pool = np.setdiff1d(np.arange(S_G), [S_EXTRA, *S_HEAVY])
    a = _sparse(np.sort(np.concatenate([rng.choice(pool, 6000 - 4, replace=False), S_HEAVY])), rng, 200.0)
    evens = np.setdiff1d(even, [S_EXTRA, *S_HEAVY])
    gal = [{} for _ in range(S_G)]
    gal[S_ROWS[1]] = {8192: 1.0}
    gal[S_ROWS[64]] = _sparse(np.sort(np.concatenate([rng.choice(evens, 62, replace=False), [0, 8192]])), rng, 20.0)
    gal[S_ROWS[65]] = _sparse(np.sort(np.concatenate([rng.choice(pool, 63, replace=False), [0, 8192]])), rng, 20.0)
    gal[S_ROWS[300]] = _sparse(np.sort(np.concatenate([rng.choice(pool, 296, replace=False), S_HEAVY])), rng, 20.0)
    return [c, b, a], gal


def shortlist(K):
    """(values float32 (3, K), rows int64 (3, K)): the four gallery rows, an empty one, and the slots -1, G and G + 1 in
    rotation (K = 1: the 65-entry row, and the 300-entry row for the 6000-entry query).  The first two queries share their
    slots."""
    rng = np.random.default_rng(K)
    vals = rng.uniform(0.1, 0.9, (3, K)).astype(np.float32)
    vals[1] = vals[0]
    if K == 1:
        return vals, np.array([[S_ROWS[65]], [S_ROWS[65]], [S_ROWS[300]]], np.int64)
    cycle = [S_ROWS[1], S_ROWS[64], -1, S_ROWS[65], S_ROWS[300], S_G, S_EMPTY, S_G + 1]
    idx = np.array([[cycle[(p + s) % len(cycle)] for p in range(K)] for s in (0, 0, 3)], np.int64)
    return vals, idx


def score_model(qrow, grow, sval, lam, bug=None):
    """s* of one slot in plain float32, as k_kr_score walks it.  Bugs: "cut_4096" - entries of V'(q) at or past 4096 are not
    seen; "lane_trip" - a lane's second trip over the gallery row never runs; "search_lo" / "search_hi" - the binary search
    never lands on the first / the last entry."""
    qc = np.array(sorted(qrow), np.int64)
    qv = np.array([qrow[c] for c in qc], np.float32)
    nq = min(len(qc), KR_SCORE_LDS) if bug == "cut_4096" else len(qc)
    gc = sorted(grow)
    mins = []
    for i, c in enumerate(gc):
        if bug == "lane_trip" and i >= WAVE:
            break
        pos = int(np.searchsorted(qc[:nq], c))
        if pos < nq and qc[pos] == c and not (bug == "search_lo" and pos == 0) and not (bug == "search_hi" and pos == nq - 1):
            mins.append(min(np.float32(grow[c]), qv[pos]))
    m = lane_sum32(np.array(mins, np.float32)) if mins else np.float32(0)
    one, lam = np.float32(1), np.float32(lam)
    dj = one - m / (np.float32(2) - m)
    return one - ((one - lam) * dj + lam * (one - np.float32(sval)))


# ---- 33 merge sources at k1 = 32, k2 = 33
L_G, L_R, K2 = 40, 4, 33


def _unit(cols, rng):
    v = rng.uniform(0.5, 1.5, len(cols))
    return dict(zip((int(c) for c in cols), v / v.sum())) if len(cols) else {}


def qe_case(bad=False):
    """(lists (4, 32) int64, own rows, gallery rows): gallery rows 0 .. 9 have disjoint columns, 10 .. 19 interleave, 20 .. 29
    hold the same twenty columns, 30 .. 39 are random (33 is empty).  List row 0 walks 0 .. 31, row 1 repeats source 7, row 2
    (whose own row is empty) walks 8 .. 39, row 3 is a permutation.  ``bad``: row 0 holds -1 and G, row 1 starts with G + 1 and
    row 3 is all pads (its V' is its own row over k2)."""
    rng = np.random.default_rng(21)
    gal = [_unit(np.arange(100 + 10 * j, 105 + 10 * j), rng) for j in range(10)]
    gal += [_unit(np.arange(j, 80, 10), rng) for j in range(10)]
    gal += [_unit(np.arange(20), rng) for _ in range(10)]
    gal += [_unit(np.sort(rng.choice(200, int(n), replace=False)), rng) for n in (3, 40, 7, 0, 64, 65, 1, 12, 90, 5)]
    own = [_unit(np.sort(rng.choice(200, n, replace=False)), rng) for n in (10, 30, 0, 70)]
    lists = np.stack([np.arange(32), np.arange(32), np.arange(8, 40), rng.permutation(L_G)[:32]]).astype(np.int64)
    lists[1, 20] = 7
    if bad:
        lists[0, 4], lists[0, 9], lists[1, 0] = -1, L_G, L_G + 1
        lists[3] = -1
    return lists, own, gal


def local_qe_model(own_row, gal, list_row, k2):
    """One V' row in plain float32, the sources added in list order."""
    G = len(gal)
    src = [own_row] + [gal[int(j)] if 0 <= j < G else {} for j in list_row[: k2 - 1]]
    out = {}
    for c in sorted(set().union(*[s.keys() for s in src])):
        acc = np.float32(0)
        for s in src:
            acc += np.float32(s.get(c, 0.0))
        out[c] = acc / np.float32(k2)
    return out


# ---- CSR rows whose offsets are not rows
def read_csr_guarded(offsets, cols, vals, nnz):
    """Rows as dicts under the kernels' rule (csr_row): [lo, hi) is a row when 0 <= lo <= hi <= nnz, otherwise it is empty."""
    out = []
    for r in range(len(offsets) - 1):
        lo, hi = int(offsets[r]), int(offsets[r + 1])
        ok = 0 <= lo <= hi <= nnz
        out.append({int(c): float(v) for c, v in zip(cols[lo:hi], vals[lo:hi])} if ok else {})
    return out


B_G = 6
BROKEN = {"hi_below_lo": (3, 7), "hi_past_nnz": (6, 27), "lo_negative": (0, -1)}      # name -> (which offset, its value)


def broken_csr(kind=None):
    """(offsets, cols, vals float32, nnz): six rows of four entries, row i holding columns 10 i .. 10 i + 3, so that rows stay
    ascending when an offset slides.  ``kind`` (a key of BROKEN) breaks one offset: row 2 ends before it starts (and row 3
    begins one entry early), row 5 ends three past nnz, or row 0 starts at -1."""
    rng = np.random.default_rng(8)
    offsets = np.arange(0, 4 * B_G + 1, 4).astype(np.int64)
    cols = np.concatenate([10 * i + np.arange(4) for i in range(B_G)]).astype(np.int32)
    v = rng.uniform(0.5, 1.5, (B_G, 4))
    vals = (v / v.sum(1, keepdims=True)).astype(np.float32).reshape(-1)
    if kind is not None:
        at, value = BROKEN[kind]
        offsets[at] = value
    return offsets, cols, vals, len(cols)
