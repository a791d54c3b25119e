"""CPU reference of the full-gallery ranking metrics (``positive_ranks`` / ``ranking_metrics``): from a (Q, G) fp32 score matrix,
labels and one excluded row per query to the rank of every positive, the average precision and the first rank.

The order is the top-k search's: an order-preserving uint32 key per score (NaN largest, -0 equal to +0), higher key first, equal
keys to the lower row.  ``brute_force`` restates the definitions pair by pair with float comparisons, without keys or a sort;
tests/test_ranking_ref.py holds the two against each other."""
import numpy as np


def score_keys(S):
    """The order-preserving uint32 key of each fp32 score: larger key = ranked earlier; NaN -> 0xffffffff, -0 -> the key of +0."""
    s = np.asarray(S, dtype=np.float32) + np.float32(0.0)             # -0 -> +0
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(s), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def _eligible(G, exclude_q, idx_offset):
    ok = np.ones(G, dtype=bool)
    if exclude_q is not None and exclude_q >= 0 and 0 <= exclude_q - idx_offset < G:
        ok[exclude_q - idx_offset] = False
    return ok


def average_precision(ranks):
    """(sum_i (i + 1) / rank_i) / R in float64, the terms added in the order i = 0, 1, ..; 0.0 without positives."""
    s = 0.0
    for i, r in enumerate(ranks):
        s += float(i + 1) / float(r)
    return s / float(len(ranks)) if len(ranks) else 0.0


def rank_positives(S, query_labels, gallery_labels, exclude=None, idx_offset=0):
    """Per query: the positives' global rows in rank order and their 1-based ranks among the eligible rows, by ONE stable sort
    on (key descending, row ascending).  Returns (offsets (Q + 1,), indices, ranks, ap (Q,) float64, first_rank (Q,) int64); a
    query without positives has ap 0 and first_rank 0."""
    S = np.asarray(S, dtype=np.float32)
    ql, gl = np.asarray(query_labels), np.asarray(gallery_labels)
    Q, G = S.shape
    keys = score_keys(S)
    offsets, indices, ranks = [0], [], []
    ap, first = np.zeros(Q, dtype=np.float64), np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        ok = _eligible(G, None if exclude is None else int(exclude[q]), idx_offset)
        rows = np.nonzero(ok)[0]
        order = rows[np.argsort(np.uint32(0xFFFFFFFF) - keys[q, rows], kind="stable")]     # rows ascend: ties to the lower row
        pos = np.nonzero(gl[order] == ql[q])[0]
        indices += (order[pos] + idx_offset).tolist()
        ranks += (pos + 1).tolist()
        offsets.append(len(indices))
        ap[q] = average_precision((pos + 1).tolist())
        first[q] = pos[0] + 1 if pos.size else 0
    return (np.asarray(offsets, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(ranks, dtype=np.int64), ap, first)


def _beats(sj, j, sp, p):
    """Whether row j with score sj ranks before row p with score sp."""
    if np.isnan(sj):
        return j < p if np.isnan(sp) else True
    if np.isnan(sp):
        return False
    if sj != sp:                       # (-0 == +0)
        return bool(sj > sp)
    return j < p


def brute_force(S, query_labels, gallery_labels, exclude=None, idx_offset=0):
    """The definitions restated: rank(p) = 1 + the eligible rows that rank before p, positives listed by ascending rank.  Same
    return value as ``rank_positives``."""
    S = np.asarray(S, dtype=np.float32)
    Q, G = S.shape
    offsets, indices, ranks = [0], [], []
    ap, first = np.zeros(Q, dtype=np.float64), np.zeros(Q, dtype=np.int64)
    for q in range(Q):
        ok = _eligible(G, None if exclude is None else int(exclude[q]), idx_offset)
        found = []
        for p in range(G):
            if ok[p] and gallery_labels[p] == query_labels[q]:
                found.append((1 + sum(1 for j in range(G) if ok[j] and j != p and _beats(S[q, j], j, S[q, p], p)), p))
        found.sort()
        indices += [p + idx_offset for _, p in found]
        ranks += [r for r, _ in found]
        offsets.append(len(indices))
        ap[q] = average_precision([r for r, _ in found])
        first[q] = found[0][0] if found else 0
    return (np.asarray(offsets, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(ranks, dtype=np.int64), ap, first)


def cmc(first_rank, R, r):
    """The share of the queries with positives whose first rank is <= r."""
    valid = np.asarray(R) > 0
    return float(((np.asarray(first_rank) <= r) & valid).sum()) / float(valid.sum())
