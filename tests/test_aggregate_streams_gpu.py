"""``aggregate`` (gem, rmac, crow, a caller's regions, ``whitening=``) on a non-blocking side stream behind a delayed input, with
the harness and in the two steps of tests/test_streams_gpu.py: the side-stream result must equal the default-stream bits, and
the same call issued on the default stream ahead of its real input must not (or the case's data could not tell the two apart).
Nothing in the aggregation reads a result back to the host - the region table travels in the kernel arguments - so the case is
declared ``syncs=False``: the harness also asserts that the call returned before its delayed input arrived."""
import functools

import pytest
import torch

import stream_cases as SC
import stream_harness as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _make(dev):
    import imageretrievalresearch_amd as M
    w = SC.whitening()                                              # 70 -> 32, fitted on the shared gallery
    p = torch.linspace(1.0, 6.0, SC.D).to(dev)

    def op(i):
        fm = i["fm"]
        return (M.aggregate(fm, "gem"), M.aggregate(fm, "gem", p=p, normalize=False), M.aggregate(fm, "rmac"),
                M.aggregate(fm, "rmac", pool="gem", return_regions=True), M.aggregate(fm, "crow"), M.aggregate(fm, "spoc"),
                M.aggregate(fm, "regions", regions=[(0, 0, 7, 10), (1, 2, 3, 3)], pool="mean"), M.aggregate(fm, "rmac", whitening=w),
                M.aggregate(i["big"], "rmac"), M.aggregate(i["big"], "crow"))
    return op, *SC.pair(dev, fm=(SC.randn, 3, SC.D, 7, 10), big=(SC.randn, 2, 9, 33, 17))


CASE = H.Case("aggregate", ("aggregate",), _make, False, True)


@functools.lru_cache(maxsize=None)
def _built():
    return H.Built(CASE, DEV)


def test_side_stream_matches_default_stream():
    b = _built()
    got = b.under_test()
    H.assert_same(got, b.expected, f"aggregate on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")


def test_a_default_stream_launch_is_detected():
    b = _built()
    got = b.control()
    assert H.differences(got, b.expected), ("aggregate: issued on the default stream ahead of its real inputs, the call still gave the "
                                            "expected bits: A and B are too alike for this case (a defect of the case's data)")
