"""``Gallery.diversify`` and ``mmr_rerank`` on a non-blocking side stream behind a delayed input, with the harness and in the two
steps of tests/test_streams_gpu.py: the side-stream result must equal the default-stream bits, and the same call issued on the
default stream ahead of its real input must not (or the case's data could not tell the two apart).  Nothing in diversify reads a
result back to the host, so the case is declared ``syncs=False``: the harness also asserts that the call returned before its
delayed input arrived."""
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
        out = []
        for dt in (torch.float32, torch.float16):
            g = M.Gallery(SC.D, dev, capacity=300, dtype=dt).add(i["r"])
            out += [g.diversify(i["q"], 5, lam=0.5, shortlist=40, stats=True),
                    g.diversify(i["q"], 5, lam=0.9, dedup=0.3, shortlist=70, block=8, stats=True),
                    g.diversify(i["q"][:2], 5, shortlist=300, exclude=i["ex"][:2], idx_offset=7)]
        return out + [M.mmr_rerank(i["q"], i["r"], 5, lam=0.5, shortlist=40)]
    return op, *SC.pair(dev, q=(SC.randn, SC.Q, SC.D), r=(SC.randn, 300, SC.D), ex=(SC.randint, 300, SC.Q))


CASE = H.Case("diversify", ("Gallery.diversify", "mmr_rerank"), _make, False, True)


@functools.lru_cache(maxsize=None)
def _built():
    return H.Built(CASE, DEV)


def test_side_stream_matches_default_stream():
    b = _built()
    got = b.under_test()
    H.assert_same(got, b.expected, f"diversify on a side stream behind a {b.delay_ms:.0f} ms delay vs the default stream")


def test_a_default_stream_launch_is_detected():
    b = _built()
    got = b.control()
    assert H.differences(got, b.expected), ("diversify: issued on the default stream ahead of its real inputs, the call still gave "
                                            "the expected bits: A and B are too alike for this case (a defect of the case's data)")
