"""Int8Gallery and FP4Gallery where their suites do not reach, on the GPU against the NumPy models (gallery_i8_ref.py,
gallery_fp4_ref.py) BIT FOR BIT: int8 sums at their ceiling (|acc_hi| near 127^2 D, above 2^24, where float(acc) rounds; D = 65536
is the GEMM's 512 k-steps), the int8 quantiser at exact ties and in its two branches only rows-as-they-are reach, galleries one
partial trip longer than the GEMV's grid, and a zero and a NaN query on the GEMV and the GEMM.  The inputs and their restated
constants are tests/quantised_extremes_cases.py; test_quantised_extremes_args.py checks every premise without a GPU.  Each
case asserts on the model what it is there for before it looks at the GPU, and every search the rank path it took."""
import numpy as np
import pytest
import torch

import gallery_fp4_ref as R4
import gallery_i8_ref as R8
import imageretrievalresearch_amd as M
import quantised_extremes_cases as C
from imageretrievalresearch_amd import Int8Gallery
from imageretrievalresearch_amd._lib import lib
from imageretrievalresearch_amd.fp4 import FP4Gallery

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_GEMM, PATH_GEMV = {"i8": 7, "fp4": 12}, {"i8": 8, "fp4": 13}
REFS, GALLERIES = {"i8": R8, "fp4": R4}, {"i8": Int8Gallery, "fp4": FP4Gallery}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_bits(got, want, what=""):
    """float32 arrays equal as int32 bit patterns; a NaN equals any NaN."""
    got, want = np.ascontiguousarray(_np(got) if torch.is_tensor(got) else got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), what
    assert (got.view(np.int32)[~gn] == want.view(np.int32)[~wn]).all(), what


def _path():
    return lib().mi355_rank_last_path() & 0xff


def _model_of(kind, x, q):
    """The kind's gallery of the rows x, and the model's planes, codes and scores of the queries q against them, from the
    library's own normalised rows; the stored codes and scales are the model's."""
    R, D = REFS[kind], x.shape[1]
    xt, qt = _dev(x), _dev(q)
    gal = GALLERIES[kind](D, DEV).add(xt)
    codes, s_g = R.quantize_rows(_np(M.l2_normalize_rows(xt)))
    hi, lo, s_q = R.query_planes(_np(M.l2_normalize_rows(qt)))
    if kind == "i8":
        assert (_np(gal.codes) == codes).all()
        _assert_bits(gal.scales, s_g, "scales")
    else:
        assert (_np(gal.codes) == R.pack(codes)[:, : (D + 1) // 2]).all()
        _assert_bits(gal.mults, s_g, "mults")
    return dict(gal=gal, q=qt, codes=codes, s_g=s_g, hi=hi, lo=lo, s_q=s_q, s=R.scores(hi, lo, s_q, codes, s_g))


def _assert_search(m, top, Q, k, what):
    v, i = m["gal"].search(m["q"][:Q], k)
    path = _path()
    _assert_bits(v, top[0][:Q, :k], what)
    assert (_np(i) == top[1][:Q, :k]).all(), what
    return path


# ---- 1. int8 sums at their ceiling
@pytest.mark.parametrize("D", C.SAT_DIMS)
def test_saturated_int8_rows_are_summed_exactly(D):
    m = _model_of("i8", C.saturated(D, C.SAT_G, D), C.saturated(D, C.SAT_Q, D + 1))
    r_hi, r_lo = C.assert_saturated(m["hi"], m["lo"], m["codes"])    # >= 0.99 of 127^2 D and of 64 * 127 D, below 2^31
    print(f"[extremes] int8 saturated D={D}: max |acc_hi| = {r_hi:.5f} of 127^2 D, max |acc_lo| = {r_lo:.5f} of 64 * 127 D")
    assert (np.abs(m["codes"][0::2, : D - 400]) == 127).all() and np.abs(m["lo"][1::2, 1: D - 30].astype(np.int32)).min() >= 63
    top = R8.topk(m["s"], C.SAT_G)
    paths = []
    for Q, k in C.SAT_CASES:
        gemv = C.i8_gemv_runs(Q, D)
        assert gemv == (Q <= 4 and D == 4096)                        # 2 * 65536 bytes of planes do not fit the GEMV's LDS
        path = _assert_search(m, top, Q, k, f"D={D} Q={Q} k={k}")
        paths.append(path)
        assert path == (PATH_GEMV["i8"] if gemv else PATH_GEMM["i8"]), (D, Q, k, path)
    print(f"[extremes] int8 saturated D={D}: paths {paths}")


# ---- 2. exact ties, and the quantiser's branches that only rows taken as they are reach
@pytest.mark.parametrize("D", [68, 70])                              # the vector and the scalar branch of the conversion
def test_int8_exact_ties_go_to_the_even_code(D):
    ties, want, scales = R8.tie_rows(D)
    n = np.concatenate([ties, np.random.default_rng(D).standard_normal((2, D)).astype(np.float32)])
    n[3, 5] = np.inf                                                 # a non-finite amax without a NaN element
    n[4] = np.float32(1e-31) * np.sign(n[4])                         # a non-zero row below 1e-30
    n[4, 1::3] *= np.float32(0.5)
    assert not np.isnan(n).any() and np.abs(n[4]).max() == np.float32(1e-31) and (n[4] != 0).all()
    gal = Int8Gallery(D, DEV)._append(_dev(n), None, normalized=True)
    codes, s = _np(gal.codes), _np(gal.scales)
    literal = [0, 2, 2, 4, 126, 126, 0, -2, -2, -4, -126, -126, 127, -127, 127, 0, 0]   # of +-(k + 0.5), +-127, 126.75, +-0.25
    for r in range(3):
        assert codes[r, :17].tolist() == literal and (codes[r] == want).all(), r
        assert (codes[r].view(np.uint8)[want == 0] == 0).all()       # -0.5 and -0.25 -> the byte 0x00
    assert s[:3].view(np.int32).tolist() == np.array([1.0, 0.125, 64.0], np.float32).view(np.int32).tolist()
    assert (s[:3] == scales).all()
    assert np.isnan(s[3]) and (codes[3] == 0).all()
    assert s[4].view(np.int32) == 0 and (codes[4] == 0).all()
    wc, ws = R8.quantize_rows(n)
    assert (codes == wc).all()
    _assert_bits(s, ws)
    assert (_np(gal._codes[:5, D:]) == 0).all()                      # the row padding


# ---- 3. the GEMV's second trip through its grid
@pytest.mark.parametrize("kind", list(C.WRAP_G))
def test_gemv_takes_a_second_trip_through_its_grid(kind):
    G = C.WRAP_G[kind]
    m = _model_of(kind, *C.wrap_case(kind))
    assert m["s"].shape == (C.WRAP_Q, G) and C.second_trip(kind, G)
    top = REFS[kind].topk(m["s"], max(C.WRAP_KS))
    C.assert_wrapped(kind, top[1])                                   # the best row, and five of the 150, lie in the second trip
    for Q in (1, 4):
        for k in C.WRAP_KS:
            path = _assert_search(m, top, Q, k, f"{kind} G={G} Q={Q} k={k}")
            assert path == PATH_GEMV[kind], (kind, Q, k, path)
    print(f"[extremes] {kind} wrap G={G}: path {PATH_GEMV[kind]}")


# ---- 4. a zero and a NaN query on both paths
@pytest.mark.parametrize("kind", list(REFS))
def test_zero_and_nan_queries(kind):
    R, G, nan_row = REFS[kind], C.SPECIAL_G, C.SPECIAL_NAN_ROW
    m = _model_of(kind, *C.special_case())
    s, gal = m["s"], m["gal"]
    others = np.arange(G) != nan_row
    assert np.isnan(s[C.NAN_Q]).all() and np.isnan(s[:, nan_row]).all() and (s[C.ZERO_Q, others].view(np.int32) == 0).all()
    paths = []
    for Q in C.SPECIAL_QS:
        assert C.ZERO_Q < Q and C.NAN_Q < Q
        for k in C.SPECIAL_KS:
            v, i = gal.search(m["q"][:Q], k)
            paths.append(_path())
            assert paths[-1] == (PATH_GEMV[kind] if Q <= 4 else PATH_GEMM[kind]), (kind, Q, k, paths[-1])
            wv, wi = R.topk(s[:Q], k)
            what = f"{kind} Q={Q} k={k}"
            _assert_bits(v, wv, what)                                # every query's bits, the special ones included
            assert (_np(i) == wi).all(), what
            v, i = _np(v), _np(i)
            assert np.isnan(v[C.NAN_Q]).all() and i[C.NAN_Q].tolist() == list(range(k)), what
            assert i[C.ZERO_Q, 0] == nan_row and np.isnan(v[C.ZERO_Q, 0]), what
            assert (v[C.ZERO_Q, 1:].view(np.int32) == 0).all() and (np.diff(i[C.ZERO_Q, 1:]) > 0).all(), what    # +0.0, ascending
            assert i[C.ZERO_Q, 1:].tolist() == [r for r in range(k) if r != nan_row][: k - 1], what
        res = gal.range_search(m["q"][:Q], 0.0)
        hit = s[:Q].astype(np.float64) >= 0.0                        # a NaN score is no hit
        rows, cols = np.nonzero(hit)
        off = np.concatenate([[0], np.cumsum(hit.sum(axis=1))])
        assert (_np(res.offsets) == off).all() and (_np(res.indices) == cols).all(), (kind, Q)
        _assert_bits(res.scores, s[:Q][rows, cols], f"{kind} Q={Q} range")
        a, b = int(off[C.ZERO_Q]), int(off[C.ZERO_Q + 1])            # the zero query: every row but the NaN row, with score +0.0
        assert _np(res.indices)[a:b].tolist() == [r for r in range(G) if r != nan_row]
        assert (_np(res.scores)[a:b].view(np.int32) == 0).all()
        assert off[C.NAN_Q + 1] == off[C.NAN_Q]                      # the NaN query: no hit
    print(f"[extremes] {kind} zero / NaN queries: paths {paths}")
