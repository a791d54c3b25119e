"""The quantised galleries' extreme cases without a GPU (tests/quantised_extremes_cases.py, the inputs of
test_quantised_extremes_gpu.py): the restated launch constants against the sources, and the premise of every case on the NumPy
models - the saturated sums reach their ceiling and round in fp32, the best rows of the wrap cases are rows of the GEMV's second
trip, and the models give a zero and a NaN query what the contract says."""
import os
import re

import numpy as np
import pytest

import gallery_fp4_ref as R4
import gallery_i8_ref as R8
import quantised_extremes_cases as C
from helpers import ROOT

F32 = np.float32
REFS = {"i8": R8, "fp4": R4}


def _src(name):
    return open(os.path.join(ROOT, "imageretrievalresearch_amd", "csrc", name)).read()


def test_restated_constants_are_the_launch_and_the_kernels():
    gemm, fp4, i8 = _src("rows_gemm.h"), _src("rank_fp4.hip"), _src("rank_i8.hip")
    blocks = re.search(r"const unsigned blocks = \(unsigned\)\(cdiv\(G, 4\) < (\d+) \? cdiv\(G, 4\) : (\d+)\);", gemm)
    assert int(blocks.group(1)) == int(blocks.group(2)) == C.GEMV_MAX_BLOCKS == 4096
    assert int(re.search(r"constexpr int GEMV_ROWS = (\d+);", fp4).group(1)) == C.FP4_GEMV_ROWS == 4
    for src in (fp4, i8):                                            # four waves per workgroup, and the stride of a trip
        assert "const i64 wave_id = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);" in src
        assert "const i64 nwaves = (i64)gridDim.x * 4;" in src
    assert "for (i64 g = wave_id; g < G; g += nwaves) {" in i8
    assert "for (i64 g0 = wave_id * GEMV_ROWS; g0 < G; g0 += nwaves * GEMV_ROWS) {" in fp4
    assert "const int nr = G - g0 < GEMV_ROWS ? (int)(G - g0) : GEMV_ROWS;" in fp4
    lds = re.search(r"constexpr size_t I8_GEMV_LDS = (\d+) \* (\d+);", i8)
    assert int(lds.group(1)) * int(lds.group(2)) == C.I8_GEMV_LDS
    assert "static bool i8_gemv(i64 Q, int ld) { return Q <= 4 && (size_t)Q * 2 * ld <= I8_GEMV_LDS; }" in i8
    assert C.GEMV_WAVES == 16384 and C.WRAP_G == {"i8": 16384 + 5, "fp4": 65536 + 5}


def test_the_wrap_cases_reach_the_second_trip():
    for kind, G in C.WRAP_G.items():
        per = C.WRAP_ROWS_PER_TRIP[kind]
        assert C.gemv_blocks(G) == C.gemv_blocks(per) == C.GEMV_MAX_BLOCKS and not C.second_trip(kind, per)   # one row fewer: one trip
        late = C.second_trip(kind, G)
        assert sorted(r for rows in late.values() for r in rows) == list(range(per, G))
        if kind == "i8":
            assert late == {w: [per + w] for w in range(5)}
        else:
            assert late == {0: [65536, 65537, 65538, 65539], 1: [65540]}                 # a whole group, and one row alone


@pytest.mark.parametrize("kind", list(C.WRAP_G))
def test_the_best_rows_of_the_wrap_cases_are_second_trip_rows(kind):
    R = REFS[kind]
    x, q = C.wrap_case(kind)
    assert x.shape == (C.WRAP_G[kind], C.WRAP_D) and q.shape == (C.WRAP_Q, C.WRAP_D)
    codes, s_g = R.quantize_rows(C.normalise(x))
    hi, lo, s_q = R.query_planes(C.normalise(q))
    v, i = R.topk(R.scores(hi, lo, s_q, codes, s_g), max(C.WRAP_KS))
    C.assert_wrapped(kind, i)
    assert (np.diff(v, axis=1) <= 0).all() and v[:, 4].min() > v[:, 5].max() + 0.1     # the five lead by a wide margin


@pytest.mark.parametrize("D", C.SAT_DIMS)
def test_saturated_int8_sums_reach_their_ceiling(D):
    x, q = C.saturated(D, C.SAT_G, D), C.saturated(D, C.SAT_Q, D + 1)
    codes, s_g = R8.quantize_rows(C.normalise(x))
    hi, lo, s_q = R8.query_planes(C.normalise(q))
    r_hi, r_lo = C.assert_saturated(hi, lo, codes)
    print(f"D={D}: max |acc_hi| = {r_hi:.5f} of 127^2 D, max |acc_lo| = {r_lo:.5f} of 64 * 127 D")
    assert (np.abs(codes[0::2, : D - 400]) == 127).all() and (np.abs(hi[0::2, : D - 30]) == 127).all()
    assert np.abs(lo[1::2, 1: D - 30].astype(np.int32)).min() >= 63
    _, _, acc_hi, acc_lo = C.saturated_sums(hi, lo, codes)
    assert np.abs(acc_hi).max() > 2 ** 24                            # float(acc_hi) rounds ...
    if D == 65536:
        assert (acc_hi.astype(F32).astype(np.int64) != acc_hi).any()  # (acc_lo, sums of +-64 * 127, keeps its low bits zero)
    s = R8.scores(hi, lo, s_q, codes, s_g)                           # ... and the model's float64 route is the fp32 fma
    t = (acc_hi.astype(F32).astype(np.float64) + acc_lo.astype(F32).astype(np.float64) / 128).astype(F32)
    assert np.array_equal(s, (t * s_q[:, None]).astype(F32) * s_g[None, :])
    assert [C.i8_gemv_runs(Q, D) for Q, _ in C.SAT_CASES] == [D == 4096 and Q <= 4 for Q, _ in C.SAT_CASES]
    assert all(k <= C.SAT_G and Q <= C.SAT_Q for Q, k in C.SAT_CASES)


@pytest.mark.parametrize("kind", list(REFS))
def test_the_models_give_a_zero_and_a_nan_query_what_the_contract_says(kind):
    R = REFS[kind]
    x, q = C.special_case()
    assert np.isnan(x).sum() == 1 and not q[C.ZERO_Q].any() and np.isnan(q[C.NAN_Q]).sum() == 1
    codes, s_g = R.quantize_rows(C.normalise(x))
    hi, lo, s_q = R.query_planes(C.normalise(q))
    assert s_q[C.ZERO_Q] == 0 and not hi[C.ZERO_Q].any() and not lo[C.ZERO_Q].any() and np.isnan(s_q[C.NAN_Q])
    s = R.scores(hi, lo, s_q, codes, s_g)
    others = np.arange(C.SPECIAL_G) != C.SPECIAL_NAN_ROW
    assert np.isnan(s[C.NAN_Q]).all() and np.isnan(s[:, C.SPECIAL_NAN_ROW]).all()
    assert (s[C.ZERO_Q, others].view(np.int32) == 0).all()           # +0.0, not -0.0
    for k in C.SPECIAL_KS:
        v, i = R.topk(s, k)
        assert i[C.NAN_Q].tolist() == list(range(k))
        assert i[C.ZERO_Q].tolist() == [C.SPECIAL_NAN_ROW] + [r for r in range(k) if r != C.SPECIAL_NAN_ROW][: k - 1]
        assert (i[:, 0] == np.where(np.arange(len(q)) == C.NAN_Q, 0, C.SPECIAL_NAN_ROW)).all()
