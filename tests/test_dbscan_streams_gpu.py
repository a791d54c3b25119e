"""``dbscan`` on a non-blocking side stream behind a delayed input, with the harness and in the two steps of
tests/test_streams_gpu.py: the side-stream result must equal the default-stream bits, and the same call issued on the default
stream ahead of its real input must not (or the case's data could not tell the two apart).  ``dbscan`` reads its cluster roots
back for the dense numbering, so the case is declared ``syncs=True``."""
import functools

import pytest
import torch

import stream_cases as SC
import stream_harness as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _make(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        g16 = M.Gallery(SC.D, dev, dtype=torch.float16).add(i["r"])
        return (M.dbscan(i["r"], 0.2, 3, block=128), M.connected_components(i["r"], 0.3), g16.dbscan(0.2, 3), g16.components(0.3))
    return op, *SC.pair(dev, r=(SC.randn, 300, SC.D))


CASE = H.Case("dbscan", ("dbscan", "connected_components", "Gallery.dbscan", "Gallery.components"), _make, True, True)


@functools.lru_cache(maxsize=None)
def _built():
    return H.Built(CASE, DEV)


def test_side_stream_matches_default_stream():
    b = _built()
    got = b.under_test()
    H.assert_same(got, b.expected, f"dbscan on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")


def test_a_default_stream_launch_is_detected():
    b = _built()
    got = b.control()
    assert H.differences(got, b.expected), ("dbscan: issued on the default stream ahead of its real inputs, the call still gave the "
                                            "expected bits: A and B are too alike for this case (a defect of the case's data)")
