"""Every workspace sizer whose layout goes through the shared host carver (``WsCarver``, csrc/common.h) returns the bytes it
returned before the carver existed: tests/golden/workspace_bytes.json holds, per sizer, a table of [arguments, bytes] recorded
from the library of the commit it names.  Callers size their scratch with these numbers, so they are part of the contract.
The sizers are host arithmetic: no GPU."""
import json
import os

import pytest

from helpers import ROOT
from imageretrievalresearch_amd import _lib

with open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_table_covers_every_carved_layout_and_names_its_commit():
    assert GOLDEN["recorded_from"].split()[0] == "9252a4e"
    names = set(GOLDEN["sizers"])
    for stem in ("rank", "rank_f16", "rank_i8", "roc_pairs", "rank_positives", "nearest_centroid", "range", "range_f16", "range_i8",
                 "cluster_members", "centroid_update", "pq_search", "ivf_scan", "ivfpq_search"):
        assert f"mi355_{stem}_workspace_bytes" in names, stem
    for name, rows in GOLDEN["sizers"].items():
        sizes = [want for _, want in rows]
        assert len(rows) >= 10 and 0 in sizes and sum(1 for s in sizes if s) >= 7, name      # legal shapes and a refused one


@pytest.mark.parametrize("name", sorted(GOLDEN["sizers"]))
def test_sizer_returns_the_recorded_bytes(name):
    fn = getattr(_lib.lib(), name)
    for args, want in GOLDEN["sizers"][name]:
        assert fn(*args) == want, (name, args)
