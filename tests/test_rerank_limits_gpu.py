"""k-reciprocal re-ranking where its loops take a second trip and where its guards decide (inputs: tests/rerank_cases.py, premises
and modelled bugs: test_rerank_limits_args.py): more rows than k_kr_scan has threads, sets of more than 128 entries, weight
rows of more than 256, V'(q) rows on both sides of the score kernel's 4096-entry LDS stage, 33 merge sources, the short last
block of knn_graph, and lists, graphs, CSR offsets and capacities that no search and no count pass produce.  Everything runs
through the staged wrappers of rerank.py against the float64 reference of tests/rerank_ref.py; every case asserts the condition
it exists for.  Buffers that hold a bad id or a broken offset are views into larger allocations whose slack is poisoned and
compared afterwards."""
import functools

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import qe_ref
import rerank_cases as C
import rerank_ref as rr
from imageretrievalresearch_amd import rerank as K
from imageretrievalresearch_amd._lib import check, lib, stream_ptr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = C.TOL       # the project's score tolerance (README: cosine scores within 1e-5), as in test_rerank_gpu.py
CERT = 5e-5       # indices must match where the reference's adjacent s* differ by more than this
Q = 37
NAN = float("nan")


def _clustered(n, D, classes, seed, spread):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(classes, D, generator=g)
    lab = torch.randint(0, classes, (n,), generator=g)
    return (centers[lab] + spread * torch.randn(n, D, generator=g)).to(DEV), lab.to(DEV)


def _np(t):
    return t.cpu().numpy()


def _rows64(gal):
    return _np(gal.data.float()).astype(np.float64)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _lens(offsets):
    return np.diff(_np(offsets))


def _report(stage, err):
    print(f"rerank limits: {stage}: worst |err| / TOL = {err / TOL:.4f}")
    return err


def _csr(rows):
    """Rows as dicts -> a device Csr with fp32 values, and the same rows with the values as the device holds them."""
    o, c, v = rr.to_csr(rows, with_vals=True)
    v = v.astype(np.float32)
    return K.Csr(_dev(o), _dev(c), _dev(v)), rr.from_csr(o, c, v)


def _same_pattern(got_offsets, got_cols, want_rows, what):
    wo, wc = rr.to_csr(want_rows)
    assert np.array_equal(_np(got_offsets), wo) and np.array_equal(_np(got_cols), wc), what


def _vals_close(got: K.Csr, want_rows, what):
    """Offsets and cols exact, vals within TOL; returns the worst error."""
    wo, wc, wv = rr.to_csr(want_rows, with_vals=True)
    assert np.array_equal(_np(got.offsets), wo) and np.array_equal(_np(got.cols), wc), what
    g = _np(got.vals).astype(np.float64)
    assert np.isfinite(g).all(), what
    err = float(np.abs(g - wv).max()) if len(wv) else 0.0
    assert err <= TOL, (what, err)
    return err


class Slack:
    """Tensors as views into larger allocations: ``put(body, poison, n)`` places n slack elements (or rows) of ``poison`` in
    front of the body and behind it, ``check()`` finds every byte of every allocation as it was."""

    def __init__(self):
        self.kept = []

    def put(self, body, poison, n=4):
        body = torch.as_tensor(np.ascontiguousarray(body)) if not torch.is_tensor(body) else body.cpu()
        slack = torch.as_tensor(poison, dtype=body.dtype).expand((n,) + tuple(body.shape[1:])).clone() if not torch.is_tensor(poison) \
            else poison.to(body.dtype)
        big = torch.cat([slack, body, slack]).to(DEV)
        self.kept.append((big, big.clone()))
        return big[len(slack):len(slack) + len(body)]

    def check(self):
        for big, was in self.kept:
            assert torch.equal(big.view(torch.uint8), was.view(torch.uint8))


# ---- k_kr_scan with two and three rows per thread
@functools.lru_cache(maxsize=None)
def _staged(G):
    """A clustered gallery of G rows at D = 16, its own graph at k1 = 5, and the float64 index built from that graph (computed
    once per G and left unchanged)."""
    x, _ = _clustered(G, 16, 20, 4, 0.5)
    gal = M.Gallery(16, DEV).add(x)
    nv, nn = gal.knn_graph(5)
    rows, nn_np = _rows64(gal), _np(nn)
    sets = rr.sets(nn_np, nn_np)
    V = rr.weights(rows, rows, sets)
    return gal, nv, nn, rows, sets, V, rr.local_qe(V, V, nn_np, 3)


@pytest.mark.parametrize("G", [1024, 1025, 2500])
def test_index_in_stages_past_one_row_per_scan_thread(G):
    k1, k2 = 5, 3
    gal, nv, nn, rows, sets, V, V2 = _staged(G)
    assert C.scan_chunk(G) == {1024: 1, 1025: 2, 2500: 3}[G] and nn.shape == (G, k1)
    nn_np = _np(nn)
    offsets, cols = K._kr_sets(nn, nn)
    _same_pattern(offsets, cols, sets, ("sets", G))
    Vg = K.Csr(offsets, cols, K._kr_weights(gal._buf, G, gal._buf, G, 16, offsets, cols))
    e1 = _vals_close(Vg, V, ("V", G))
    V2g = K._kr_local_qe(nn, k2, Vg, Vg, G)
    e2 = _vals_close(V2g, V2, ("V'", G))
    # query rows: the gallery's own rows with themselves excluded, so both count passes scan R rows as well
    R = min(G, 1025)
    assert C.scan_chunk(R) == min(C.scan_chunk(G), 2)
    sv, si = gal.search(gal.data[:R].contiguous(), k1, exclude=torch.arange(R, dtype=torch.int64, device=DEV))
    tau = nv[:, -1].contiguous()
    qo, qc = K._kr_sets(si, nn, sv, tau)
    qsets = rr.sets(_np(si), nn_np, _np(sv), _np(tau))
    _same_pattern(qo, qc, qsets, ("query sets", G))
    Vq = K.Csr(qo, qc, K._kr_weights(gal._buf, R, gal._buf, G, 16, qo, qc))
    Vq_ref = rr.weights(rows[:R], rows, qsets)
    e3 = _vals_close(Vq, Vq_ref, ("V(q)", G))
    Vq2 = K._kr_local_qe(si, k2, Vq, Vg, G)
    e4 = _vals_close(Vq2, rr.local_qe(Vq_ref, V, _np(si), k2), ("V'(q)", G))
    _report(f"staged index G={G} (V, V', V(q), V'(q))", max(e1, e2, e3, e4))


def test_batches_of_3_and_1025_rows_give_the_same_rows():
    k1, k2, G, R = 5, 3, 1025, 1025
    gal, nv, nn, *_ = _staged(G)
    assert C.scan_chunk(R) == 2
    offsets, cols = K._kr_sets(nn, nn)
    Vg = K.Csr(offsets, cols, K._kr_weights(gal._buf, G, gal._buf, G, 16, offsets, cols))
    sv, si = gal.search(gal.data[:R].contiguous(), k1, exclude=torch.arange(R, dtype=torch.int64, device=DEV))
    tau = nv[:, -1].contiguous()
    qo, qc = K._kr_sets(si, nn, sv, tau)
    Vq = K.Csr(qo, qc, K._kr_weights(gal._buf, R, gal._buf, G, 16, qo, qc))
    Vq2 = K._kr_local_qe(si, k2, Vq, Vg, G)

    def cut(csr, a, b):
        lo, hi = int(csr[0][a]), int(csr[0][b])
        return (csr[0][a:b + 1] - lo,) + tuple(t[lo:hi] for t in csr[1:])

    for a in (0, 511, 1022):                                         # the first thread's run, a middle one, the last rows
        b = a + 3
        so, sc = K._kr_sets(si[a:b].contiguous(), nn, sv[a:b].contiguous(), tau)
        want = cut((qo, qc), a, b)
        assert torch.equal(so, want[0]) and torch.equal(sc, want[1]), a
        own = K.Csr(so, sc, cut(Vq, a, b)[2].contiguous())
        small = K._kr_local_qe(si[a:b].contiguous(), k2, own, Vg, G)
        assert all(torch.equal(x, y) for x, y in zip(small, cut(Vq2, a, b))), a


# ---- end to end above 1024 rows
E2E_CASES = [(1025, 16, 4, 0.5), (2500, 70, 3, 2.0)]


@pytest.mark.parametrize("kind", ["fp32", "fp16"])
@pytest.mark.parametrize("G, D, seed, spread", E2E_CASES)
def test_rerank_above_1024_rows_against_float64(G, D, seed, spread, kind):
    """The reference is fed this gallery's own round-1 lists, as in test_rerank_gpu.py.  With float64 lists the reference
    certifies 37 of 37 queries in both cases (smallest gap among ranks 1 .. k + 1: 8.2e-5 at G = 1025, 1.1e-4 at G = 2500; seeds
    1 .. 8 scanned on the CPU, these have the widest gaps).  On the MI355X's own lists all 37 are certified as well: smallest gap
    8.2e-5 / 1.4e-4 (G = 1025, fp32 / fp16 rows) and 1.1e-4 / 1.2e-4 (G = 2500)."""
    k, k1, k2, lam, Ks = 5, 20, 6, 0.3, 100
    assert C.scan_chunk(G) >= 2
    x, _ = _clustered(G + Q, D, 20, seed, spread)
    gal = M.Gallery(D, DEV, dtype=torch.float16 if kind == "fp16" else torch.float32).add(x[:G])
    q = x[G:]
    index = gal.rerank_index(k1, k2)
    assert index.V.offsets.shape == (G + 1,)
    sstar, sv, si, nv, nn = K._rerank_scores(gal, q, k1, k2, lam, Ks, None)
    qn = qe_ref.normalize(_np(q))
    ref = rr.pipeline(qn, _rows64(gal), _np(index.nv), _np(index.nn), _np(nv), _np(nn), _np(sv), _np(si), k2, lam)
    err = float(np.abs(_np(sstar).astype(np.float64) - ref).max())
    gap = rr.gaps(ref, k)
    cert = gap > CERT
    print(f"rerank limits: end to end G={G} D={D} {kind}: worst |err| / TOL = {err / TOL:.4f}, certified {int(cert.sum())} of {Q}, "
          f"smallest gap {gap.min():.2e}")
    assert err <= TOL, (G, D, kind, err)
    vals, idx = gal.rerank(q, k, k1=k1, k2=k2, lam=lam, shortlist=Ks)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.shape == idx.shape == (Q, k)
    rv, ri, _ = rr.rank_shortlist(ref, _np(si), k)
    assert (~cert).mean() <= 0.02, (G, D, kind, int((~cert).sum()))
    assert np.array_equal(_np(idx)[cert], ri[cert]), (G, D, kind)
    assert np.abs(_np(vals) - rv).max() <= TOL


# ---- the 193-entry set
def test_a_set_of_193_entries_and_33_merge_sources():
    g = C.graph193()
    graph = _dev(g)
    offsets, cols = K._kr_sets(graph, graph)
    want = rr.sets(g, g)
    _same_pattern(offsets, cols, want, "R* of the hand-made graph")
    lens = _lens(offsets)
    assert lens[0] == 193 and lens.max() > 2 * C.WAVE and (lens > C.WAVE).sum() == 20 and lens.max() <= C.MAX_ROW
    qsets = None
    for equal, below in ((None, None), (5, None), (None, 5)):
        lists, vals, tau = C.query193(equal, below)
        qo, qc = K._kr_sets(_dev(lists), graph, _dev(vals), _dev(tau))
        qwant = rr.sets(lists, g, vals, tau)
        _same_pattern(qo, qc, qwant, ("query rows", equal, below))
        ql = _lens(qo)
        if below is None:
            assert ql[0] == 192 > 2 * C.WAVE and (qsets is None or qwant == qsets)
            qsets, qoff, qcols = qwant, qo, qc
        else:
            # one step below tau row 5 is no member: neither it nor its 11 circulant neighbours (now 11 of 17 in R) expand
            assert qwant != qsets and ql[0] == 192 - 1 - 12 * 5
    # weights and the 33-source merge over those sets
    k2 = C.K2
    x = C.unit_rows(C.G193, 70, 5)
    xq = C.unit_rows(C.G193, 70, 6)
    rows, qrows = _dev(x), _dev(xq)
    Vg = K.Csr(offsets, cols, K._kr_weights(rows, C.G193, rows, C.G193, 70, offsets, cols))
    V = rr.weights(x.astype(np.float64), x.astype(np.float64), want)
    e1 = _vals_close(Vg, V, "V over the 193-row graph")
    V2g = K._kr_local_qe(graph, k2, Vg, Vg, C.G193)
    e2 = _vals_close(V2g, rr.local_qe(V, V, g, k2), "V' at k2 = 33")
    Vq = K.Csr(qoff, qcols, K._kr_weights(qrows, C.G193, rows, C.G193, 70, qoff, qcols))
    Vq_ref = rr.weights(xq.astype(np.float64), x.astype(np.float64), qsets)
    e3 = _vals_close(Vq, Vq_ref, "V(q) over the 193-row graph")
    Vq2 = K._kr_local_qe(graph, k2, Vq, Vg, C.G193)
    e4 = _vals_close(Vq2, rr.local_qe(Vq_ref, V, g, k2), "V'(q) at k2 = 33")
    assert _lens(V2g.offsets).max() > 2 * C.WAVE and k2 == C.MAX_K1 + 1
    _report("193-entry set (V, V', V(q), V'(q) at k2 = 33)", max(e1, e2, e3, e4))


def test_33_hand_made_merge_sources():
    lists, own, gal = C.qe_case()
    own_d, own32 = _csr(own)
    gal_d, gal32 = _csr(gal)
    assert lists.shape[1] == C.MAX_K1 and C.K2 == 33 and list(lists[1]).count(7) == 2 and not own[2]
    out = K._kr_local_qe(_dev(lists), C.K2, own_d, gal_d, C.L_G)
    err = _vals_close(out, rr.local_qe(own32, gal32, lists, C.K2), "33 sources")
    assert _lens(out.offsets).max() > 2 * C.WAVE
    one = K._kr_local_qe(_dev(lists), 1, own_d, gal_d, C.L_G)       # k2 = 1: the own rows, the empty one included, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(one, own_d))
    _report("33 hand-made merge sources", err)


# ---- weights on the hand-made patterns
@functools.lru_cache(maxsize=None)
def _weight_rows(D):
    return C.unit_rows(C.W_G, D, 1), C.unit_rows(len(C.W_LENGTHS), D, 2)


def _weights_check(rows_t, gal_t, G, D, offsets, cols, what):
    """_kr_weights against the reference on the rows as stored; every non-empty row sums to 1."""
    vals = K._kr_weights(rows_t, len(offsets) - 1, gal_t, G, D, _dev(offsets), _dev(cols))
    sets = [cols[offsets[r]:offsets[r + 1]] for r in range(len(offsets) - 1)]
    want = rr.to_csr(rr.weights(_np(rows_t[:, :D].double()), _np(gal_t[:G, :D].double()), sets), with_vals=True)[2]
    got = _np(vals).astype(np.float64)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    assert err <= TOL, (what, err)
    sums = np.add.reduceat(got, offsets[:-1][np.diff(offsets) > 0])
    assert np.abs(sums - 1.0).max() <= TOL, what
    return err


@pytest.mark.parametrize("rows_dtype, gal_dtype", [(torch.float32, torch.float32), (torch.float16, torch.float16),
                                                   (torch.float16, torch.float32), (torch.float32, torch.float16)])
@pytest.mark.parametrize("D", C.W_DIMS)
def test_weight_rows_past_a_sum_trip_and_a_division_trip(D, rows_dtype, gal_dtype):
    offsets, cols = C.weight_pattern()
    lens = np.diff(offsets)
    assert lens.max() > 2 * C.THREADS and {0, C.WAVE + 1, C.THREADS + 1} <= set(lens.tolist()) and D <= C.KR_MAX_DIM
    gal, rows = _weight_rows(D)
    err = _weights_check(_dev(rows).to(rows_dtype), _dev(gal).to(gal_dtype), C.W_G, D, offsets, cols, (D, rows_dtype, gal_dtype))
    _report(f"weights D={D} rows {str(rows_dtype)[6:]} gallery {str(gal_dtype)[6:]}", err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_weights_scalar_path_at_a_dim_the_vector_path_would_take(dtype):
    D = 64
    offsets, cols = C.weight_pattern()
    gal, rows = _weight_rows(D)
    big = torch.full((C.W_G, D + 1), NAN, dtype=dtype, device=DEV)  # the column behind every row is poison
    big[:, :D] = _dev(gal).to(dtype)
    view = big[:, :D]
    elem = big.element_size()
    assert D % 8 == 0 and view.stride(0) == D + 1 and (view.stride(0) * elem) % 16 != 0 and view.data_ptr() % 16 == 0
    err = _weights_check(_dev(rows).to(dtype), view, C.W_G, D, offsets, cols, ("ld = dim + 1", dtype))
    packed = K._kr_weights(_dev(rows).to(dtype), len(C.W_LENGTHS), view.contiguous(), C.W_G, D, _dev(offsets), _dev(cols))
    strided = K._kr_weights(_dev(rows).to(dtype), len(C.W_LENGTHS), view, C.W_G, D, _dev(offsets), _dev(cols))
    assert float((packed - strided).abs().max()) <= TOL             # the vector path on the same rows, another order of sums
    _report(f"weights ld = dim + 1 at dim 64, {str(dtype)[6:]}", err)


# ---- score on both sides of 4096
@functools.lru_cache(maxsize=None)
def _score_case():
    qrows, gal = C.score_case()
    return _csr(qrows), _csr(gal)


@pytest.mark.parametrize("Ks", [1, 5, 100])
def test_score_rows_of_4096_4097_and_6000_entries(Ks):
    (qd, q32), (gd, g32) = _score_case()
    nq = _lens(qd.offsets)
    assert nq.tolist() == [C.KR_SCORE_LDS, C.KR_SCORE_LDS + 1, 6000] and nq[1] > 4096 and gd.offsets.shape == (C.S_G + 1,)
    vals, idx = C.shortlist(Ks)
    out = _np(K._kr_score(qd, gd, C.S_G, _dev(vals), _dev(idx), C.S_LAM))
    want = rr.scores(q32, g32, vals, idx, C.S_LAM)
    pad = (idx < 0) | (idx >= C.S_G)
    assert np.array_equal(np.isneginf(out), pad) and np.array_equal(np.isneginf(want), pad) and not np.isnan(out).any()
    if Ks > 1:
        assert pad.any() and (idx == C.S_G).any() and (idx == -1).any() and not pad.all()
    err = float(np.abs(out[~pad].astype(np.float64) - want[~pad]).max())
    assert err <= TOL, (Ks, err)
    # the staged row and the same row plus one unmatched entry, read where it lies: the same sums, the same bits
    assert np.array_equal(out[0].view(np.int32), out[1].view(np.int32))
    _report(f"score K={Ks}", err)


# ---- the guards
GRAPH_POISON = torch.arange(C.K1, dtype=torch.int64).expand(4, -1)  # slack rows that list 0 .. 31: reciprocal to all of them


def test_guards_of_the_sets():
    G = C.G193
    gb = C.graph193_bad()
    s = Slack()
    graph = s.put(gb, GRAPH_POISON)
    offsets, cols = K._kr_sets(graph, graph)
    want = rr.sets(gb, gb)
    _same_pattern(offsets, cols, want, "gallery rows with bad ids")
    assert _lens(offsets)[0] == 192 and int(cols.min()) >= 0 and int(cols.max()) < G
    lists, vals, tau = C.query193_bad()
    qo, qc = K._kr_sets(s.put(lists, GRAPH_POISON), graph, s.put(vals, float("inf")), s.put(tau, float("-inf")))
    _same_pattern(qo, qc, rr.sets(lists, gb, vals, tau), "query rows with bad ids")
    assert _lens(qo)[2] == 0 and int(qc.min()) >= 0 and int(qc.max()) < G
    s.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guards_of_the_weights(dtype):
    D = 64                                                          # the vector path: 16-byte loads of the rows
    offsets, cols = C.weight_pattern(bad=True)
    assert {-1, C.W_G, C.W_G + 1} <= set(cols.tolist())
    gal, rows = _weight_rows(D)
    s = Slack()
    gal_t = s.put(torch.as_tensor(gal).to(dtype), NAN)              # NaN rows where -1, G and G + 1 point
    cols_t = s.put(cols, 0)
    vals = K._kr_weights(_dev(rows).to(dtype), len(C.W_LENGTHS), gal_t, C.W_G, D, _dev(offsets), cols_t)
    sets = [cols[offsets[r]:offsets[r + 1]] for r in range(len(C.W_LENGTHS))]
    want = rr.to_csr(rr.weights(_np(_dev(rows).to(dtype).double()), _np(gal_t.double()), sets), with_vals=True)
    assert np.array_equal(want[1], cols)
    got = _np(vals).astype(np.float64)
    assert np.isfinite(got).all()
    err = float(np.abs(got - want[2]).max())
    assert err <= TOL, err
    bad = (cols < 0) | (cols >= C.W_G)
    assert (got[bad] == 0).all() and (got[~bad] > 0).all()
    s.check()
    _report(f"weights with bad columns, {str(dtype)[6:]}", err)


def _guarded_csr(s, rows, lead=3, tail=5):
    """The rows as a device Csr whose cols and vals begin with ``lead`` and end with ``tail`` entries of no row (column 0 with
    the value 1000), inside allocations with the same poison around them; the offsets start at ``lead`` and their slack makes
    row -1 the leading entries and rows G and G + 1 the trailing ones.  Returns (Csr, the rows with fp32 values)."""
    o, c, v = rr.to_csr(rows, with_vals=True)
    v = v.astype(np.float32)
    c2 = np.concatenate([np.zeros(lead, np.int32), c, np.zeros(tail, np.int32)])
    v2 = np.concatenate([np.full(lead, 1e3, np.float32), v, np.full(tail, 1e3, np.float32)])
    end = int(o[-1]) + lead
    front = torch.zeros(4, dtype=torch.int64)
    back = torch.tensor([end + 2, end + tail, end + tail, end + tail], dtype=torch.int64)
    big = torch.cat([front, torch.as_tensor(o + lead), back]).to(DEV)
    s.kept.append((big, big.clone()))
    return K.Csr(big[4:4 + len(o)], s.put(c2, 0), s.put(v2, 1e3)), rr.from_csr(o, c, v)


def test_guards_of_the_local_expansion():
    lists, own, gal = C.qe_case(bad=True)
    assert {-1, C.L_G, C.L_G + 1} <= set(lists.reshape(-1).tolist()) and (lists[3] == -1).all()
    s = Slack()
    own_d, own32 = _guarded_csr(s, own)
    gal_d, gal32 = _guarded_csr(s, gal)
    out = K._kr_local_qe(s.put(lists, GRAPH_POISON), C.K2, own_d, gal_d, C.L_G)
    err = _vals_close(out, rr.local_qe(own32, gal32, lists, C.K2), "33 sources with bad ids")
    s.check()
    _report("local expansion with bad ids", err)


def test_guards_of_the_score():
    (qd0, q32), (gd0, g32) = _score_case()
    qrows, gal = C.score_case()
    s = Slack()
    qd, _ = _guarded_csr(s, qrows)
    gd, _ = _guarded_csr(s, gal)
    vals, idx = C.shortlist(5)
    assert {-1, C.S_G, C.S_G + 1} <= set(idx.reshape(-1).tolist())
    out = K._kr_score(qd, gd, C.S_G, s.put(vals, 0.5), s.put(idx, torch.full((4, 5), C.S_ROWS[300], dtype=torch.int64)), C.S_LAM)
    plain = K._kr_score(qd0, gd0, C.S_G, _dev(vals), _dev(idx), C.S_LAM)
    assert torch.equal(out, plain)                                  # where the rows lie changes nothing
    want = rr.scores(q32, g32, vals, idx, C.S_LAM)
    pad = (idx < 0) | (idx >= C.S_G)
    assert np.array_equal(np.isneginf(_np(out)), pad)
    err = float(np.abs(_np(out)[~pad].astype(np.float64) - want[~pad]).max())
    assert err <= TOL, err
    s.check()
    _report("score with bad slots", err)


@pytest.mark.parametrize("kind", sorted(C.BROKEN))
def test_broken_offsets_read_as_empty_rows(kind):
    k1, k2, lam = 3, 3, 0.3
    o, c, v, nnz = C.broken_csr()
    ob, _, _, _ = C.broken_csr(kind)
    good = C.read_csr_guarded(o, c, v, nnz)
    broken = C.read_csr_guarded(ob, c, v, nnz)
    at = C.BROKEN[kind][0]
    assert broken != good and any(not r for r in broken) and all(good) and ob[at] != o[at]
    s = Slack()
    col_t, val_t = s.put(c, 0), s.put(v, 1e3)                       # what lies before entry 0 and past nnz is poison
    ok_d = K.Csr(_dev(o), col_t, val_t)
    bad_d = K.Csr(s.put(ob, 0), col_t, val_t)
    lists = np.array([[(r + 1 + t) % C.B_G for t in range(k1)] for r in range(C.B_G)], np.int64)
    sv = np.random.default_rng(4).uniform(0.1, 0.9, (C.B_G, C.B_G)).astype(np.float32)
    si = np.tile(np.arange(C.B_G, dtype=np.int64), (C.B_G, 1))
    worst = 0.0
    for own_d, own_r, gal_d, gal_r in ((bad_d, broken, ok_d, good), (ok_d, good, bad_d, broken)):
        out = K._kr_local_qe(_dev(lists), k2, own_d, gal_d, C.B_G)
        want = rr.local_qe(own_r, gal_r, lists, k2)
        worst = max(worst, _vals_close(out, want, (kind, "local_qe")))
        sc = _np(K._kr_score(own_d, gal_d, C.B_G, _dev(sv), _dev(si), lam))
        assert np.isfinite(sc).all()
        err = float(np.abs(sc.astype(np.float64) - rr.scores(own_r, gal_r, sv, si, lam)).max())
        assert err <= TOL, (kind, "score", err)
        worst = max(worst, err)
    s.check()
    _report(f"broken offsets ({kind})", worst)


def test_a_row_that_does_not_fit_is_not_written():
    """The fill passes with a capacity one short of the last row's end, and the sets' fill with offsets that are not the count
    pass's: the row stays as it was, every other row is written, nothing behind the capacity is touched."""
    slack = 8
    # sets
    g = C.graph193()
    graph = _dev(g)
    offsets, cols = K._kr_sets(graph, graph)
    nnz, o = cols.numel(), _np(offsets)
    st = stream_ptr(torch.device(DEV))

    def fill_sets(offs, cap):
        buf = torch.full((nnz + slack,), C.SENTINEL, dtype=torch.int32, device=DEV)
        check(lib().mi355_kr_sets(graph.data_ptr(), None, None, C.G193, C.K1, graph.data_ptr(), C.G193, offs.data_ptr(),
                                  buf.data_ptr(), cap, st))
        return buf

    full = fill_sets(offsets, nnz)
    assert torch.equal(full[:nnz], cols) and bool((full[nnz:] == C.SENTINEL).all())
    short = fill_sets(offsets, nnz - 1)
    last = int(o[-2])
    assert nnz - last == 2                                           # the last row: a leaf and its owner
    assert torch.equal(short[:last], cols[:last]) and bool((short[last:] == C.SENTINEL).all())
    moved = offsets.clone()
    moved[1] -= 1                                                    # row 0 one entry short, row 1 one entry long
    wrong = fill_sets(moved, nnz)
    two = int(o[2])
    assert bool((wrong[:two] == C.SENTINEL).all()) and torch.equal(wrong[two:nnz], cols[two:]) and o[1] == 193
    # the local expansion
    lists, own, gal = C.qe_case()
    own_d, _ = _csr(own)
    gal_d, _ = _csr(gal)
    lists_t = _dev(lists)
    ref = K._kr_local_qe(lists_t, C.K2, own_d, gal_d, C.L_G)
    n2, o2 = ref.cols.numel(), _np(ref.offsets)

    def fill_qe(cap):
        oc = torch.full((n2 + slack,), C.SENTINEL, dtype=torch.int32, device=DEV)
        ov = torch.full((n2 + slack,), float(C.SENTINEL), dtype=torch.float32, device=DEV)
        check(lib().mi355_kr_local_qe(lists_t.data_ptr(), C.L_R, C.K1, C.K2, own_d.offsets.data_ptr(), own_d.cols.data_ptr(),
                                      own_d.vals.data_ptr(), own_d.cols.numel(), gal_d.offsets.data_ptr(), gal_d.cols.data_ptr(),
                                      gal_d.vals.data_ptr(), gal_d.cols.numel(), C.L_G, ref.offsets.data_ptr(), oc.data_ptr(),
                                      ov.data_ptr(), cap, st))
        return oc, ov

    oc, ov = fill_qe(n2)
    assert torch.equal(oc[:n2], ref.cols) and torch.equal(ov[:n2], ref.vals) and bool((oc[n2:] == C.SENTINEL).all())
    oc, ov = fill_qe(n2 - 1)
    last = int(o2[-2])
    assert n2 - last > 1                                             # a row of many entries: none of them is written
    assert torch.equal(oc[:last], ref.cols[:last]) and torch.equal(ov[:last], ref.vals[:last])
    assert bool((oc[last:] == C.SENTINEL).all()) and bool((ov[last:] == C.SENTINEL).all())


# ---- knn_graph: the short last block
@pytest.mark.parametrize("G, block", [(258, 256), (260, 256), (261, 256), (23, 1), (23, 5), (23, 7)])
def test_knn_graph_block_edges(G, block):
    k1 = 5
    x, _ = _clustered(G, 16, 5, 9, 0.5)
    gal = M.Gallery(16, DEV).add(x)
    rest = G % max(block, 5)
    assert rest == {(258, 256): 2, (260, 256): 4, (261, 256): 5, (23, 1): 3, (23, 5): 3, (23, 7): 2}[(G, block)]
    assert (1 <= rest <= 4) == ((G, block) != (261, 256))           # the short last block re-searches the last five rows
    nv, nn = K.knn_graph(gal, k1, block)
    ex = torch.arange(G, dtype=torch.int64, device=DEV)
    v, i = gal.search(gal.data, k1, exclude=ex)
    assert torch.equal(nn, i) and torch.equal(nv.view(torch.int32), v.view(torch.int32)), (G, block)
    assert bool((nn != ex[:, None]).all()) and int(nn.min()) >= 0 and int(nn.max()) < G
