"""NumPy model of the graph index: ``merged_graph`` (the adjacency of forward lists and their reverse edges) and the beam walk of
``mi355_graph_search``, step for step as include/mi355_retrieval.h states it.  The walk takes the score matrix ``S`` (Q, G) as
input (on the GPU tests: the scores ``mi355_rescore_candidates`` gives every pair), so that the model fixes every index, every
score bit and both counters, and nothing of the arithmetic."""
import math

import numpy as np


def beam_key(score, row):
    """Sort key of the beam order (that of merge_topk): NaN first, then descending score (-0 equal to +0), ties to the lower
    row."""
    s = float(score)
    if math.isnan(s):
        return (0, 0.0, int(row))
    return (1, -s + 0.0, int(row))           # + 0.0: -(+0.0) = -0.0 becomes +0.0 (they compare equal anyway)


def merged_graph(fwd, degree):
    """(G, degree) int32: slots [0, h) = fwd[r]; slots [h, degree) = the rows s with r in fwd[s] that are not in fwd[r], ordered
    by (the first position of r in fwd[s], s), cut to degree - h; -1 where nothing is left."""
    fwd = np.asarray(fwd, np.int64)
    G, h = fwd.shape
    assert degree == 2 * h
    out = np.full((G, degree), -1, np.int32)
    out[:, :h] = fwd
    rev = [[] for _ in range(G)]
    for s in range(G):
        seen = set()
        for pos in range(h):
            r = int(fwd[s, pos])
            if 0 <= r < G and r not in seen:
                seen.add(r)
                rev[r].append((pos, s))
    for r in range(G):
        mine = set(int(x) for x in fwd[r])
        keep = [s for _, s in sorted(rev[r]) if s not in mine][: degree - h]
        out[r, h: h + len(keep)] = keep
    return out


def walk(s_row, graph, seeds, k, ef, max_iters, eligible=None, idx_offset=0):
    """One query: (values (k,) float32, indices (k,) int64, iters, visited).  ``s_row`` (G,) float32 scores of the query,
    ``graph`` (G, R) ints, ``seeds`` (nseed,) ints, ``eligible`` (G,) bool or None.  An id outside [0, G) other than -1 raises."""
    G, R = graph.shape
    visited = set()
    beam = []                                               # [key, row, expanded], sorted by key

    def offer(rows):
        nonlocal beam
        for n in rows:
            n = int(n)
            if n == -1:
                continue
            if not 0 <= n < G:
                raise ValueError(f"id {n} outside [0, {G})")
            if n in visited:
                continue
            visited.add(n)
            beam.append([beam_key(s_row[n], n), n, False])
        beam = sorted(beam, key=lambda e: e[0])[:ef]

    offer(seeds)
    iters = 0
    for _ in range(max_iters):
        p = next((e for e in beam if not e[2]), None)
        if p is None:
            break
        p[2] = True
        iters += 1
        offer(graph[p[1]])
    vals = np.full(k, -np.inf, np.float32)
    idx = np.full(k, -1, np.int64)
    got = [e[1] for e in beam if eligible is None or eligible[e[1]]][:k]
    for i, r in enumerate(got):
        vals[i], idx[i] = s_row[r], r + idx_offset
    return vals, idx, iters, len(visited)


def search(S, graph, seeds, k, ef, max_iters, eligible=None, idx_offset=0):
    """Every query of ``S`` (Q, G): (values (Q, k) float32, indices (Q, k) int64, iters (Q,) int32, visited (Q,) int32)."""
    S, graph, seeds = np.asarray(S, np.float32), np.asarray(graph), np.asarray(seeds)
    Q = S.shape[0]
    out = [walk(S[q], graph, seeds[q], k, ef, max_iters, None if eligible is None else eligible[q], idx_offset) for q in range(Q)]
    return (np.stack([o[0] for o in out]).reshape(Q, k), np.stack([o[1] for o in out]).reshape(Q, k),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.int32))


def eligible_mask(Q, G, query_labels=None, gallery_labels=None, label_filter=None, exclude=None, idx_offset=0):
    """(Q, G) bool: the rows the filter of the filtered searches accepts for every query."""
    ok = np.ones((Q, G), bool)
    if label_filter is not None:
        same = np.asarray(query_labels)[:, None] == np.asarray(gallery_labels)[None, :]
        ok &= same if label_filter == "same" else ~same
    if exclude is not None:
        ex = np.asarray(exclude)
        ok &= ~((np.arange(G)[None, :] + idx_offset == ex[:, None]) & (ex[:, None] >= 0))
    return ok


def topk_exact(s_row, k):
    """The exhaustive top-k of one query in beam order: (values, indices)."""
    order = sorted(range(len(s_row)), key=lambda r: beam_key(s_row[r], r))[:k]
    return np.asarray([s_row[r] for r in order], np.float32), np.asarray(order, np.int64)
