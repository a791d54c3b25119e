"""Exact reference of the selection layer (csrc/rank.hip: k_topk_small*, k_topk_bitonic*, k_clear_pads, k_pack_candidates,
k_unpack_candidates, k_hit_counts, k_distinct_topn), numpy only.  Nothing here rounds: every result is defined exactly.

Order of candidates (include/mi355_retrieval.h): NaN first (NaN is the largest value, two NaNs tie), then the higher value
(-0 == +0), then the LOWER index.  It is written as one ``np.lexsort`` over explicit keys; ``oracle.rank.topk_rows`` sorts
``-S`` and so puts NaN last, which is why it is not used for these cases.

"No candidate": an explicit index at or above ``NO_CANDIDATE`` = 2**62 - the int64 maximum ``IDX_PAD`` that the kernels
leave in unfilled slots, and the shard pad 2**62.  Such an entry's value is ignored, it never takes a slot while a real
candidate is left, and the slots that stay empty come back as (-inf, IDX_PAD) (a filtered search: (-inf, -1))."""
import numpy as np

IDX_PAD = np.iinfo(np.int64).max
NO_CANDIDATE = np.int64(1) << np.int64(62)
NEG_INF_BITS = np.uint32(0xFF800000)
LABEL_ANY, LABEL_SAME, LABEL_DIFFERENT = 0, 1, 2


def bits(x):
    """The uint32 bit patterns of float32 values."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def select_topk(vals, idx, k, idx_offset=0, return_pos=False):
    """Top-k of every row of ``vals`` (Q, n) float32 with indices ``idx`` (Q, n) int64, or ``arange(n) + idx_offset`` when
    ``idx`` is None.  Returns (values (Q, k) float32, indices (Q, k) int64); values are the input's own bits.  With
    ``return_pos`` also the column each slot came from (-1: an empty slot)."""
    vals = np.asarray(vals, dtype=np.float32)
    Q, n = vals.shape
    assert 1 <= k <= n, (k, n)
    if idx is None:
        idx = np.broadcast_to(np.arange(n, dtype=np.int64) + np.int64(idx_offset), (Q, n))
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.shape == vals.shape
    missing = idx >= NO_CANDIDATE
    nan = np.isnan(vals)
    not_nan = ~nan
    neg = np.where(nan, np.float32(0), -(vals + np.float32(0)))       # ascending -v = descending v; -0 and +0 tie
    order = np.lexsort((idx, neg, not_nan, missing), axis=-1)[:, :k]   # last key first: real, NaN, value, index
    out_v = np.take_along_axis(vals, order, 1).copy()
    out_i = np.take_along_axis(idx, order, 1).copy()
    empty = np.take_along_axis(missing, order, 1)
    out_v[empty] = -np.inf
    out_i[empty] = IDX_PAD
    if return_pos:
        return out_v, out_i, np.where(empty, -1, order)
    return out_v, out_i


def eligible(Q, n, idx_offset=0, exclude=None, query_labels=None, gallery_labels=None, mode=LABEL_ANY):
    """(Q, n) bool: row j (global index j + idx_offset) is eligible for query q (mi355_rank_filter)."""
    ok = np.ones((Q, n), bool)
    if exclude is not None:
        ex = np.asarray(exclude, np.int64)
        loc = np.where(ex >= 0, ex - np.int64(idx_offset), -1)
        ok &= np.arange(n, dtype=np.int64)[None, :] != loc[:, None]
    if mode != LABEL_ANY:
        same = np.asarray(gallery_labels, np.int64)[None, :] == np.asarray(query_labels, np.int64)[:, None]
        ok &= same if mode == LABEL_SAME else ~same
    return ok


def select_filtered(vals, k, idx_offset=0, exclude=None, query_labels=None, gallery_labels=None, mode=LABEL_ANY):
    """``select_topk`` over the eligible rows only; the slots they do not fill are (-inf, -1)."""
    vals = np.asarray(vals, dtype=np.float32)
    Q, n = vals.shape
    idx = np.broadcast_to(np.arange(n, dtype=np.int64) + np.int64(idx_offset), (Q, n)).copy()
    idx[~eligible(Q, n, idx_offset, exclude, query_labels, gallery_labels, mode)] = IDX_PAD
    v, i = select_topk(vals, idx, k)
    return clear_pads(v, i, np.iinfo(np.int64).min, IDX_PAD)


def clear_pads(vals, idx, lo, hi):
    """Entries whose index lies outside [lo, hi) become (-inf, -1) (k_clear_pads)."""
    vals, idx = np.array(vals, dtype=np.float32), np.array(idx, dtype=np.int64)
    out = (idx < lo) | (idx >= hi)
    vals[out] = -np.inf
    idx[out] = -1
    return vals, idx


def pack(vals, idx, Q, k):
    """mi355_pack_candidates: (Q, kk) results (None: kk = 0) -> (Q, k, 2) int32 {f32 bits, LOCAL int32 index}; slots
    j >= kk are {bits(-inf), -1}."""
    out = np.empty((Q, k, 2), np.int32)
    out[:, :, 0] = NEG_INF_BITS.view(np.int32)
    out[:, :, 1] = -1
    if vals is not None:
        kk = vals.shape[1]
        assert kk <= k
        out[:, :kk, 0] = bits(vals).view(np.int32)
        out[:, :kk, 1] = np.asarray(idx, np.int64).astype(np.int32)
    return out


def unpack(packed, offsets):
    """The candidate lists mi355_merge_packed_topk merges: (world, Q, k, 2) int32 -> values, indices (Q, world * k), shard
    r's offset added to its local indices, a slot with local index < 0 = no candidate."""
    packed = np.ascontiguousarray(packed, dtype=np.int32)
    world, Q, k, _ = packed.shape
    v = packed[..., 0].view(np.float32)
    loc = packed[..., 1].astype(np.int64)
    gi = np.where(loc >= 0, loc + np.asarray(offsets, np.int64)[:, None, None], NO_CANDIDATE)
    return (np.ascontiguousarray(v.transpose(1, 0, 2)).reshape(Q, world * k),
            np.ascontiguousarray(gi.transpose(1, 0, 2)).reshape(Q, world * k))


def unpack_merge(packed, offsets, k):
    """mi355_merge_packed_topk: the k best of the world * k candidates of every query; empty slots (-inf, IDX_PAD)."""
    v, i = unpack(packed, offsets)
    return select_topk(v, i, k)


def hit_counts(idx, query_cls, gallery_cls):
    """(top-1 hits, top-min(3, k) hits); an index outside [0, G) is a miss."""
    idx = np.asarray(idx, np.int64)
    gc, qc = np.asarray(gallery_cls, np.int64), np.asarray(query_cls, np.int64)
    G = gc.shape[0]
    head = idx[:, :3]
    real = (head >= 0) & (head < G)
    hit = real & (gc[np.where(real, head, 0)] == qc[:, None])
    return int(hit[:, 0].sum()), int(hit.any(1).sum())


def distinct_topn(idx, val, gallery_cls, n):
    """The first n distinct classes along each ranked list, indices outside [0, G) skipped: (classes, indices, values)
    (Q, n), unfilled slots (-1, -1, NaN)."""
    idx, val = np.asarray(idx, np.int64), np.asarray(val, np.float32)
    gc = np.asarray(gallery_cls, np.int64)
    Q, k = idx.shape
    oc = np.full((Q, n), -1, np.int64)
    oi = np.full((Q, n), -1, np.int64)
    ov = np.full((Q, n), np.nan, np.float32)
    for q in range(Q):
        seen = []
        for j in range(k):
            g = idx[q, j]
            if len(seen) == n:
                break
            if g < 0 or g >= gc.shape[0] or gc[g] in seen:
                continue
            oc[q, len(seen)], oi[q, len(seen)], ov[q, len(seen)] = gc[g], g, val[q, j]
            seen.append(gc[g])
    return oc, oi, ov


def assert_selection_equal(v, i, want_v, want_i, what=""):
    """Indices equal; values: NaN at the same positions, every other position numerically equal (tolerance zero)."""
    v, i = np.asarray(v), np.asarray(i)
    np.testing.assert_array_equal(i, want_i, err_msg=f"{what}: indices")
    np.testing.assert_array_equal(np.isnan(v), np.isnan(want_v), err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(np.where(np.isnan(v), np.float32(0), v), np.where(np.isnan(want_v), np.float32(0), want_v),
                                  err_msg=f"{what}: values")
