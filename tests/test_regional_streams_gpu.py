"""``RegionGallery.add`` / ``scores`` / ``search`` / ``rerank`` / ``pooled`` and ``maxsim`` on a non-blocking side stream behind a
delayed input, with the harness and in the two steps of tests/test_streams_gpu.py: the side-stream result must equal the
default-stream bits, and the same call issued on the default stream ahead of its real input must not (or the case's data could
not tell the two apart).  Nothing in regional.py reads a result back to the host, so the case is declared ``syncs=False``: the
harness also asserts that the call returned before its delayed input arrived."""
import functools

import pytest
import torch

import stream_cases as SC
import stream_harness as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, R, RQ, NQ = 60, 6, 5, 9


def _make(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        rg = M.RegionGallery(SC.D, R, dev, capacity=10).add(i["g"][:20], i["ex"][:20]).add(i["g"][20:])   # grows on the stream
        out = [rg.data, rg.nbytes, rg.query_codes(i["q"]), rg.scores(i["q"]), rg.scores(i["q"], i["idx"], weights=i["w"], matches=True),
               rg.search(i["q"], 7, weights=i["w"]), rg.search(i["q"][:2], ROWS, exclude=i["ex"][:2] + 5, idx_offset=5)]
        for dt in (torch.float32, torch.float16):
            gal = rg.pooled(dt)
            qg = M.RegionGallery(SC.D, RQ, dev).add(i["q"]).pooled().data
            out += [gal.data, rg.rerank(gal, qg, i["q"], 5, shortlist=20, matches=True),
                    rg.rerank(gal, qg[:2], i["q"][:2], 3, weights=i["w"][:2], exclude=i["ex"][:2] + 5, idx_offset=5)]
        return out + [M.maxsim(i["q"], i["g"], i["w"])]
    return op, *SC.pair(dev, g=(SC.randn, ROWS, R, SC.D), q=(SC.randn, NQ, RQ, SC.D), w=(SC.randn, NQ, RQ), ex=(SC.randint, ROWS, ROWS),
                        idx=(SC.randint, ROWS, NQ, 33))


CASE = H.Case("regional", ("RegionGallery", "RegionGallery.add", "RegionGallery.data", "RegionGallery.query_codes", "RegionGallery.scores",
                           "RegionGallery.search", "RegionGallery.rerank", "RegionGallery.pooled", "maxsim"), _make, False, True)


@functools.lru_cache(maxsize=None)
def _built():
    return H.Built(CASE, DEV)


def test_side_stream_matches_default_stream():
    b = _built()
    got = b.under_test()
    H.assert_same(got, b.expected, f"regional on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")


def test_a_default_stream_launch_is_detected():
    b = _built()
    got = b.control()
    assert H.differences(got, b.expected), ("regional: issued on the default stream ahead of its real inputs, the call still gave "
                                            "the expected bits: A and B are too alike for this case (a defect of the case's data)")
