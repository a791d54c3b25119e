"""NumPy model of the IVF search over an int8 gallery (mi355_ivf_scan_i8, Int8IVFIndex), bit for bit: a score is the int8
score of gallery_i8_ref (quantize_rows / query_planes / scores) for the pair, the rows a query sees are those of its probed
lists (ivf_ref: lists_of / probed_rows / eligible), the candidate slab is laid out as the header says, and the selection is the
library's (gallery_i8_ref.topk with a mask: NaN first, ties to the lower GALLERY row, pads (-inf, -1))."""
import numpy as np

import gallery_i8_ref as R8
import ivf_ref as I

F32 = np.float32
NO_CAND = I.NO_CAND


def pair_scores(qn, codes, s_g):
    """float32 [Q][G]: the score of every (query, row) pair from the normalised float32 queries qn and the gallery's codes and
    scales - the bits of the exhaustive search and of the scan alike."""
    hi, lo, s_q = R8.query_planes(qn)
    return R8.scores(hi, lo, s_q, np.asarray(codes), np.asarray(s_g, dtype=F32))


def probed_mask(G, offsets, order, probes):
    """bool [Q][G]: the rows of the lists each query probes."""
    mask = np.zeros((len(probes), G), bool)
    for q, p in enumerate(probes):
        mask[q, I.probed_rows(offsets, order, p)] = True
    return mask


def slab(s, offsets, order, probes, cap, ok=None, idx_offset=0):
    """(cand_val float32 [Q][cap], cand_idx int64 [Q][cap]) from the pair scores s: the rows of probes[q][0], then
    probes[q][1], ... fill slots 0 .. n_q - 1 in list order with (score, row + idx_offset); an ineligible row (ok [Q][G] False)
    and every slot from n_q on hold (-inf, 2^62)."""
    Q = len(probes)
    val = np.full((Q, cap), -np.inf, F32)
    idx = np.full((Q, cap), NO_CAND, np.int64)
    for q in range(Q):
        r = I.probed_rows(offsets, order, probes[q])
        assert r.size <= cap
        keep = np.ones(r.size, bool) if ok is None else ok[q, r]
        val[q, :r.size] = np.where(keep, s[q, r], F32(-np.inf))
        idx[q, :r.size] = np.where(keep, r + idx_offset, NO_CAND)
    return val, idx


def search(s, offsets, order, probes, k, ok=None, idx_offset=0):
    """(values float32 [Q][k], indices int64 [Q][k]) of the index's search: the top-k of each query's probed, eligible rows."""
    mask = probed_mask(s.shape[1], offsets, order, probes)
    if ok is not None:
        mask &= ok
    v, i = R8.topk(s, k, mask)
    return v, np.where(i >= 0, i + idx_offset, -1)


def refined(shortlist_idx, dots32, k, idx_offset=0):
    """The refined search from the int8 shortlist's indices [Q][R] (pads -1): re-ranked by the float32 dot the rescoring
    routine gives the pair (dots32 [Q][G]; NaN first, ties to the lower row), which is also the value; pads (-inf, -1)."""
    Q = shortlist_idx.shape[0]
    wi = np.full((Q, k), -1, np.int64)
    wv = np.full((Q, k), -np.inf, F32)
    for q in range(Q):
        c = shortlist_idx[q][shortlist_idx[q] >= 0] - idx_offset
        key = np.where(np.isnan(dots32[q, c]), np.inf, dots32[q, c].astype(np.float64))
        c = c[np.lexsort((c, -key))][:k]
        wi[q, :c.size], wv[q, :c.size] = c + idx_offset, dots32[q, c]
    return wv, wi
