"""The long-row cases without a GPU (tests/long_rows_cases.py, the inputs of test_long_rows_gpu.py): the float64 reference
leaves the tolerance to the kernels - a plain float32 dot of the same operands stays within a tenth of SCORE_TOL of it at every
dim used - and each bug the GPU tests are there to catch moves some score of every case it applies to by more than ten times
SCORE_TOL.  Also the restated constants: the group size of the IVF scan per dim (over int8 rows: against the constants and the
rule read from ivf.hip), and which side of its LDS rule every GEMV case lies on."""
import os
import re

import numpy as np
import pytest

import ivf_ref
import long_rows_cases as C
from helpers import ROOT, SCORE_TOL

KINDS = ("f16", "f32")


def _operands(kind, D, G, Q):
    """(float64 normalised queries, float64 rows as stored, float32 queries, float32 rows) of one case."""
    rows = C.stored(kind, C.raw(kind, 1, G, D))
    x = C.raw(kind, 2, Q, D)
    return ivf_ref.normalise(x), rows.astype(np.float64), ivf_ref.normalise(x).astype(np.float32), rows


def _all_dims(kind):
    gemv = C.GEMV_F16 if kind == "f16" else C.GEMV_F32
    return sorted(set(C.RESCORE_DIMS[kind]) | set(C.IVF_DIMS[kind]) | {D for D, _ in gemv})


@pytest.mark.parametrize("kind", KINDS)
def test_a_float32_dot_leaves_nine_tenths_of_the_tolerance(kind):
    for D in _all_dims(kind):
        qn, rows, q32, r32 = _operands(kind, D, 200, 9)
        err = float(np.abs((q32 @ r32.T).astype(np.float64) - qn @ rows.T).max())
        print(f"{kind} D={D}: max |float32 dot - f64| {err:.3e}")
        assert err <= SCORE_TOL / 10, (kind, D, err)


@pytest.mark.parametrize("kind", KINDS)
def test_a_dropped_or_repeated_trip_shows(kind):
    first = C.FIRST_TRIP[kind]
    applied = 0
    for D in _all_dims(kind):
        qn, rows, _, _ = _operands(kind, D, 200, 9)
        S = qn @ rows.T
        if D == first:                                               # one trip exactly: nothing to drop
            assert np.array_equal(C.cut_after_first_trip(qn, rows, kind), S)
            continue
        assert D > first
        for bug in (C.cut_after_first_trip, C.second_trip_rereads_first):
            moved = float(np.abs(bug(qn, rows, kind) - S).max())
            assert moved > 10 * SCORE_TOL, (kind, D, bug.__name__, moved)
            applied += 1
    assert applied >= 2 * (len(_all_dims(kind)) - 1)


@pytest.mark.parametrize("kind", KINDS)
def test_a_group_row_one_unit_early_shows(kind):
    applied = 0
    for D in C.IVF_DIMS[kind]:
        nq = C.ivf_nq(D, kind)
        qn, rows, _, _ = _operands(kind, D, C.IVF_G, C.IVF_Q)
        S = qn @ rows.T
        B = C.last_query_one_unit_early(qn, rows, kind, nq)
        lasts = [g[-1] for g in C.ivf_groups(nq) if len(g) >= 2]
        if nq == 1:
            assert not lasts and np.array_equal(B, S)                # single queries: no neighbour
            continue
        for q in lasts:
            moved = float(np.abs(B[q] - S[q]).max())
            assert moved > 10 * SCORE_TOL, (kind, D, q, moved)
        others = [q for q in range(C.IVF_Q) if q not in lasts]
        assert np.array_equal(B[others], S[others])
        applied += 1
    assert applied == 5                                              # every dim with a group of 4, 3 or 2


def test_the_group_size_steps_where_the_cases_say():
    for kind in KINDS:
        got = {D: C.ivf_nq(D, kind) for D in C.IVF_DIMS[kind]}
        assert got == {D: C.IVF_NQ[D] for D in C.IVF_DIMS[kind]}, kind
        assert sorted(set(got.values())) == [1, 2, 3, 4]
        assert C.ivf_nq(C.TOO_LONG, kind) == 0 and C.ldq(C.TOO_LONG, kind) * 4 > 64 * 1024 >= C.ldq(16384, kind) * 4
    assert [len(g) for g in C.ivf_groups(4)] == [4, 4, 1] and [len(g) for g in C.ivf_groups(3)] == [3, 3, 3]
    assert [len(g) for g in C.ivf_groups(2)] == [2, 2, 2, 2, 1] and [len(g) for g in C.ivf_groups(1)] == [1] * 9
    assert sum(C.IVF_LENGTHS) == 200 and 0 in C.IVF_LENGTHS and sorted(C.IVF_PROBES) == list(range(5))
    assert (np.bincount(C.ivf_assign(), minlength=5) == C.IVF_LENGTHS).all()


def test_the_int8_group_size_is_the_rule_of_the_scan():
    """The restated rule against the constants and the expression of ivf.hip, and every step of it against the cases."""
    csrc = os.path.join(ROOT, "imageretrievalresearch_amd", "csrc")
    src, quant = open(os.path.join(csrc, "ivf.hip")).read(), open(os.path.join(csrc, "i8_quant.h")).read()
    assert int(re.search(r"constexpr int IVF_NQ_I8 = (\d+);", src).group(1)) == C.IVF_MAXQ_I8 == 8
    lds = re.search(r"constexpr size_t IVF_LDS = (\d+) \* (\d+);", src)
    assert int(lds.group(1)) * int(lds.group(2)) == C.IVF_LDS == 65536
    assert int(re.search(r"constexpr int I8_KSTEP = (\d+);", quant).group(1)) == C.I8_SEGMENT == 128
    assert "(dim + I8_KSTEP - 1) / I8_KSTEP * I8_KSTEP" in quant
    rule = src[src.index("static int ivf_group_i8(int lq)"):src.index("static bool ivf_shape_ok")]
    assert "const size_t fit = IVF_LDS / ((size_t)2 * lq);" in rule
    assert "return (int)(fit < (size_t)IVF_NQ_I8 ? fit : (size_t)IVF_NQ_I8);" in rule
    assert "const int lq = i8_ld(dim), nq = ivf_group_i8(lq);" in src and "const size_t lds = (size_t)nq * 2 * lq;" in src
    got = {D: C.ivf_nq_i8(D) for D in C.IVF_DIMS_I8}
    assert got == C.IVF_GROUP_I8 == {4096: 8, 4100: 7, 8192: 4, 8200: 3, 16384: 2, 16400: 1, 32768: 1}
    assert [C.lq_i8(D) for D in C.IVF_DIMS_I8] == [4096, 4224, 8192, 8320, 16384, 16512, 32768]
    for nq, split in C.IVF_SPLIT_I8.items():
        assert [len(g) for g in C.ivf_groups(nq)] == split and sum(split) == C.IVF_Q == 9
    assert sorted(C.IVF_SPLIT_I8) == sorted(set(got.values())) == [1, 2, 3, 4, 7, 8]
    assert C.ivf_nq_i8(32768) * 2 * C.lq_i8(32768) == C.IVF_LDS and C.ivf_nq_i8(32769) == 0      # the whole 64 KB; past it
    assert all(D > C.FIRST_TRIP["i8"] for D in C.IVF_DIMS_I8[1:]) and C.IVF_DIMS_I8[0] == C.FIRST_TRIP["i8"]


def test_every_gemv_rule_has_a_case_on_either_side():
    assert C.GEMV_F16[(4160, 3)] and not C.GEMV_F16[(4160, 4)] and C.GEMV_F16[(4096, 4)]
    assert all(C.GEMV_F16[(D, Q)] for D in (2048, 2112, 4096) for Q in (1, 2, 3, 4))
    assert C.GEMV_F32 == {(D, Q): Q * D * 4 <= 60 * 1024 for D, Q in C.GEMV_F32}
    assert C.GEMV_I8[(8192, 4)] and not C.GEMV_I8[(8320, 4)] and C.GEMV_I8[(8320, 1)]
    # every kind has a dim of one trip exactly, one a unit (its gallery's row padding) past it, and several trips
    assert {2048, 2112} <= {D for D, _ in C.GEMV_F16} and {4096, 4224} <= {D for D, _ in C.GEMV_I8}
    assert all(D % 64 == 0 for D, _ in C.GEMV_F16) and all(D % 128 == 0 for D, _ in C.GEMV_I8)
