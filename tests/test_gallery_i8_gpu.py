"""int8 resident gallery on the GPU: the conversion, every search path, the filters and the range search against the NumPy
model of the contract (gallery_i8_ref.py) BIT FOR BIT - the integer dot products are exact, so there is no tolerance and no
tie slack anywhere - plus the properties the other galleries are tested for (a score depends on its query and row only)."""
import ctypes

import numpy as np
import pytest
import torch

import gallery_i8_ref as R
import imageretrievalresearch_amd as M
from imageretrievalresearch_amd import Int8Gallery, MI355Error
from imageretrievalresearch_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_I8_GEMM, PATH_I8_GEMV, FUSED, BITONIC = 7, 8, 0x100, 0x200
NQ = 200                                                            # queries of every model; each Q of a test is a prefix


def _randn(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _assert_bits(got, want, what=""):
    """float32 arrays equal as int32 bit patterns; a NaN equals any NaN."""
    got, want = np.ascontiguousarray(_np(got) if torch.is_tensor(got) else got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.int32)[~gn] == want.view(np.int32)[~wn]).all(), what


_models = {}


def _model(D, G, labels=False):
    """A seeded gallery of G rows, its Int8Gallery, NQ queries and the model's scores and full order, once per (D, G)."""
    key = (D, G, labels)
    if key not in _models:
        x, q = _randn((G, D), 100 + D + G), _randn((NQ, D), 200 + D + G)
        gl = torch.randint(0, 50, (G,), generator=torch.Generator().manual_seed(D + G)).to(DEV) if labels else None
        gal = Int8Gallery(D, DEV).add(x, gl)
        codes, s_g = R.quantize_rows(_np(M.l2_normalize_rows(x)))
        hi, lo, s_q = R.query_planes(_np(M.l2_normalize_rows(q)))
        s = R.scores(hi, lo, s_q, codes, s_g)
        assert (_np(gal.codes) == codes).all()
        _assert_bits(gal.scales, s_g, "scales")
        _models[key] = dict(x=x, q=q, gal=gal, s=s, top=R.topk(s, min(1024, G)), gl=gl)
    return _models[key]


# ---- 1. conversion
@pytest.mark.parametrize("D", [1, 70, 128, 129, 1536])
def test_conversion_bit_for_bit(D):
    x = _randn((1000, D), D)
    x[3] = 0.0
    x[10, D // 2] = float("nan")
    x[20] = 0.0
    x[20, D - 1] = -2.5                                              # one non-zero element
    x[30] = 0.37 * torch.where(torch.arange(D, device=DEV) % 3 == 0, -1.0, 1.0)   # equal magnitudes: every code +-127
    x[40] = 1e-9 * x[41]                                             # norm below eps
    gal = Int8Gallery(D, DEV, capacity=1)
    cap0 = gal._codes.shape[0]
    for a, b in ((0, 1), (1, 300), (300, 301), (301, 1000)):
        gal.add(x[a:b])
    assert len(gal) == 1000 and gal._codes.shape[0] > cap0           # the buffers grew with a resident row in them
    codes, scales = R.quantize_rows(_np(M.l2_normalize_rows(x)))
    assert np.isnan(scales[10]) and scales[3] == 0 and (np.abs(codes[30]) == 127).all() and np.abs(codes[40]).max() == 127
    assert gal.codes.shape == (1000, D) and gal.codes.dtype == torch.int8 and gal.scales.shape == (1000,)
    assert (_np(gal.codes) == codes).all()
    _assert_bits(gal.scales, scales)
    ld = (D + 127) // 128 * 128
    assert gal._codes.shape[1] == ld and (gal._codes[:1000, D:] == 0).all()
    assert gal.nbytes == gal._codes.shape[0] * (ld + 4)
    assert lib().mi355_gallery_i8_bytes(1000, D) == 1000 * ld
    live = ~np.isnan(scales)
    assert torch.equal(gal.dequantized()[torch.from_numpy(live).to(DEV)],
                       torch.from_numpy(codes[live].astype(np.float32) * scales[live, None]).to(DEV))


# ---- 2. every search path equals the model
@pytest.mark.parametrize("G", [1, 127, 129, 1000, 5000])
@pytest.mark.parametrize("D", [1, 70, 128, 200, 300, 400, 1536])     # 1, 1, 1, 2, 3, 4, 12 k-steps: the gallery ring is 3 deep
def test_search_equals_the_model(D, G):
    m = _model(D, G)
    for Q in (1, 3, 4, 5, 64, 65, 200):
        for k in (1, 3, 8, 9, 150, 1024):
            if k > G:
                continue
            v, i = m["gal"].search(m["q"][:Q], k)
            path = lib().mi355_rank_last_path()
            what = f"D={D} G={G} Q={Q} k={k}"
            _assert_bits(v, m["top"][0][:Q, :k], what)
            assert (_np(i) == m["top"][1][:Q, :k]).all(), what
            if Q <= 4:
                assert path & 0xff == PATH_I8_GEMV, what
            else:
                assert path == PATH_I8_GEMM | (FUSED if k <= 8 else BITONIC), what


# ---- 3. the seam between the two launches
@pytest.mark.parametrize("k", [3, 150])
def test_tail_launch_is_bit_identical(k):
    """Q = 200 x G = 5000 is 2 x 40 tiles: 8 slots cut them into whole rounds (one launch), 12 slots leave a tail launch.
    D = 200, 300, 400: two, three and four k-steps."""
    out = (ctypes.c_int * 5)()
    for D in (200, 300, 400):
        m = _model(D, 5000)
        want_v, want_i = m["gal"].search(m["q"], k)
        try:
            for slots, tail in ((8, False), (12, True)):
                assert lib().mi355_rank_set_round_slots(slots) == 0
                v, i = m["gal"].search(m["q"], k)
                assert lib().mi355_rank_last_tiles(out, 5) == 5
                assert out[0] == slots and (out[3] > 0) == tail, list(out)
                assert torch.equal(v.view(torch.int32), want_v.view(torch.int32)) and torch.equal(i, want_i), D
        finally:
            assert lib().mi355_rank_set_round_slots(0) == 0
        _assert_bits(want_v, m["top"][0][:, :k], f"D={D}")
        assert (_np(want_i) == m["top"][1][:, :k]).all(), D


# ---- 4. a score depends on its query and its row only
@pytest.mark.parametrize("k", [3, 150])
def test_scores_do_not_depend_on_the_batch(k):
    m = _model(1536, 5000)
    gal, q = m["gal"], m["q"]
    v, i = gal.search(q, k)
    for a, b in ((0, 1), (0, 4), (3, 8), (0, 64), (60, 200)):
        pv, pi = gal.search(q[a:b], k)
        assert torch.equal(pv.view(torch.int32), v[a:b].view(torch.int32)) and torch.equal(pi, i[a:b]), (a, b)
    ov, oi = gal.search(q, k, idx_offset=1000)
    assert torch.equal(ov.view(torch.int32), v.view(torch.int32)) and torch.equal(oi, i + 1000)
    rv, ri = gal.search(q, k)
    assert torch.equal(rv.view(torch.int32), v.view(torch.int32)) and torch.equal(ri, i)
    ev, ei = gal.search(q[:0], 5)
    assert ev.shape == (0, 5) and ei.shape == (0, 5)


# ---- 5. ties and NaN
@pytest.mark.parametrize("Q", [1, 64])
def test_duplicates_ascend_and_nan_ranks_first(Q):
    D, G = 1536, 3000
    x = _randn((G, D), 5)
    for r in (17, 40, 2999):
        x[r] = x[5]
    x[7] = float("nan")
    q = x[5:6].repeat(Q, 1) + 1e-3 * _randn((Q, D), 9)
    q[0] = x[5]
    v, i = Int8Gallery(D, DEV).add(x).search(q, 8)
    assert torch.isnan(v[:, 0]).all() and (i[:, 0] == 7).all()
    assert i[0, 1:5].tolist() == [5, 17, 40, 2999]                   # equal scores: ascending index
    assert torch.equal(v[0, 1:5].view(torch.int32), v[0, 1:2].view(torch.int32).expand(4))


# ---- 6. filters
def _eligible(m, Q, ql, label_filter, exclude):
    G = m["s"].shape[1]
    ok = np.ones((Q, G), bool)
    if label_filter is not None:
        same = _np(ql)[:, None] == _np(m["gl"])[None, :]
        ok &= same if label_filter == "same" else ~same
    if exclude is not None:
        ex = _np(exclude)
        ok[np.arange(Q)[ex >= 0], ex[ex >= 0]] = False
    return ok


@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("Q", [3, 70])
def test_filtered_search_equals_the_model(Q, k):
    m = _model(200, 3000, labels=True)
    gal, q = m["gal"], m["q"][:Q]
    gen = torch.Generator().manual_seed(Q * 100 + k)
    ql = torch.randint(0, 50, (Q,), generator=gen).to(DEV)
    ql[1] = 999                                                      # no row has this label: "same" leaves only pads
    ex = torch.randint(-5, 3000, (Q,), generator=gen).to(DEV)
    padded = False
    for lf, e in (("same", None), ("different", None), (None, ex), ("same", ex), ("different", ex)):
        v, i = gal.search(q, k, query_labels=ql if lf else None, label_filter=lf, exclude=e)
        ok = _eligible(m, Q, ql, lf, e)
        wv, wi = R.topk(m["s"][:Q], k, mask=ok)
        _assert_bits(v, wv, (lf, e is not None))
        assert (_np(i) == wi).all(), (lf, e is not None)
        padded = padded or (wi == -1).any()
    assert padded
    v, i = gal.search(q, k, query_labels=ql, label_filter="same")
    assert (i[1] == -1).all() and torch.isinf(v[1]).all() and (v[1] < 0).all()
    bare = Int8Gallery(200, DEV).add(m["x"][:100])
    with pytest.raises(MI355Error, match="needs gallery labels"):
        bare.search(q, k, query_labels=ql, label_filter="same")
    with pytest.raises(MI355Error, match="needs gallery labels"):
        M.Gallery(200, DEV).add(m["x"][:100]).search(q, k, query_labels=ql, label_filter="same")


# ---- 7. range search
@pytest.mark.parametrize("Q", [2, 70])
def test_range_search_equals_the_model(Q):
    m = _model(200, 3000, labels=True)
    gal, q, s = m["gal"], m["q"][:Q], m["s"][:Q]
    keep = max(1, s.size // 100)
    thr_some = float(np.partition(s.ravel(), s.size - keep)[s.size - keep])      # a score itself: >= keeps it
    ql = torch.randint(0, 50, (Q,), generator=torch.Generator().manual_seed(Q)).to(DEV)
    ex = torch.arange(Q, device=DEV) * 7
    for thr, kw, ok in ((thr_some, {}, np.ones(s.shape, bool)),
                        (float(s.max()) + 1e-3, {}, np.ones(s.shape, bool)),
                        (thr_some, dict(query_labels=ql, label_filter="different", exclude=ex), _eligible(m, Q, ql, "different", ex))):
        res = gal.range_search(q, thr, **kw)
        hit = ok & (s.astype(np.float64) >= thr)
        rows, cols = np.nonzero(hit)                                 # row-major: queries in order, rows ascending
        off = np.concatenate([[0], np.cumsum(hit.sum(axis=1))])
        assert (_np(res.offsets) == off).all() and res.offsets.dtype == torch.int64
        assert (_np(res.indices) == cols).all() and res.indices.dtype == torch.int64
        _assert_bits(res.scores, s[rows, cols])
    assert int(gal.range_search(q, thr_some).offsets[-1]) >= keep
    assert gal.range_search(q, float(s.max()) + 1e-3).indices.numel() == 0
    want = M.Gallery(200, DEV).add(m["x"]).range_search(q, 2.0)      # the layout of Gallery.range_search's result
    got = gal.range_search(q, 2.0)
    assert type(got) is type(want) and [t.shape for t in got] == [t.shape for t in want]


# ---- 8. Gallery.quantized(), recall and the error cases
def test_quantized_equals_add_and_recall():
    D, G, Q = 128, 20000, 256
    x, q = _randn((G, D), 31), _randn((Q, D), 32)
    lab = torch.arange(G, device=DEV) % 97
    exact = M.Gallery(D, DEV).add(x, lab)
    a, b = Int8Gallery(D, DEV).add(x, lab), exact.quantized()
    assert isinstance(b, Int8Gallery) and len(b) == G
    assert torch.equal(a.codes, b.codes) and torch.equal(a.scales.view(torch.int32), b.scales.view(torch.int32))
    assert torch.equal(b.labels, lab) and b.labels.data_ptr() != exact.labels.data_ptr()
    with pytest.raises(MI355Error):
        M.Gallery(D, DEV, dtype=torch.float16).add(x[:10]).quantized()
    mean, per = b.recall(q, 10, exact)
    print(f"recall@10 of the int8 search against the fp32 gallery: {mean:.4f}")
    assert per.shape == (Q,) and per.dtype == torch.float64
    assert mean >= 0.95
    with pytest.raises(MI355Error, match="embedding dims differ"):
        a.search(q[:, :64], 3)
    with pytest.raises(MI355Error, match="selected index k out of range"):
        Int8Gallery(D, DEV).add(x[:5]).search(q, 6)
    with pytest.raises(MI355Error, match="gallery rows must be"):
        a.add(x[:, :64])


def test_queries_on_another_device_are_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    gal = Int8Gallery(16, DEV).add(_randn((10, 16), 1))
    with pytest.raises(MI355Error, match="queries on"):
        gal.search(torch.zeros(2, 16, device="cuda:1"), 1)
