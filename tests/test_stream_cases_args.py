"""CPU checks of the stream tests' own machinery: the table covers every public entry (or says why not), its syncs list is
documented, and the leaf walker / bit comparison of tests/stream_harness.py tell equal from different.  No GPU is touched."""
import inspect
import os
import re
from typing import NamedTuple

import pytest
import torch

import stream_cases as SC
import stream_harness as H
from helpers import ROOT


def _public_members(cls):
    """The public methods, class / static methods and properties a class defines itself (not what it inherits)."""
    out = []
    for name, v in vars(cls).items():
        if name.startswith("_"):
            continue
        if callable(v) or isinstance(v, (property, classmethod, staticmethod)):
            out.append(name)
    return out


def _public_entries():
    import imageretrievalresearch_amd as M
    from imageretrievalresearch_amd.models import MI355Model
    names = list(M.__all__)
    classes = {"Gallery": M.Gallery, "Int8Gallery": M.Int8Gallery, "PreparedGallery": M.PreparedGallery, "IVFIndex": M.IVFIndex,
               "RerankIndex": M.RerankIndex, "Whitening": M.Whitening, "ShardedGallery": M.ShardedGallery, "Model": MI355Model}
    for prefix, cls in classes.items():
        names += [f"{prefix}.{m}" for m in _public_members(cls)]
    return names


def _covered(cases=None):
    return {c for case in (SC.CASES if cases is None else cases) for c in case.covers}


def _uncovered(cases=None):
    covered = _covered(cases)
    return [n for n in _public_entries() if n not in covered and n not in SC.HOST_ONLY and n not in SC.NEEDS_PROCESS_GROUP]


def test_every_public_entry_has_a_case_or_a_reason():
    assert _uncovered() == [], f"public entries without a stream case (add one to tests/stream_cases.py): {_uncovered()}"


def test_no_entry_is_in_two_places():
    covered = _covered()
    for name in _public_entries():
        places = [name in covered, name in SC.HOST_ONLY, name in SC.NEEDS_PROCESS_GROUP]
        assert sum(places) == 1, f"{name}: has a case / HOST_ONLY / NEEDS_PROCESS_GROUP = {places}"
    known = set(_public_entries())
    for name in list(SC.HOST_ONLY) + list(SC.NEEDS_PROCESS_GROUP):
        assert name in known, f"{name} is excused but is no public entry (renamed or removed?)"
    for name, reason in list(SC.HOST_ONLY.items()) + list(SC.NEEDS_PROCESS_GROUP.items()):
        assert reason and "\n" not in reason, name


def test_deleting_a_case_names_the_uncovered_entry():
    only = [c for c in SC.CASES if "merge_topk" in c.covers]
    assert len(only) == 1
    left = [c for c in SC.CASES if c is not only[0]]
    assert _uncovered(left) == ["merge_topk"]


def test_case_names_are_unique_and_every_case_with_inputs_has_a_control():
    names = [c.name for c in SC.CASES]
    assert len(set(names)) == len(names)
    assert [c.name for c in SC.CASES if not c.control] == ["synth_fill"]          # the one case without a device input


def test_syncs_flags_agree_with_the_syncing_list():
    syncing = set(SC.SYNCING)
    assert syncing <= _covered()
    for c in SC.CASES:
        hit = syncing & set(c.covers)
        if c.syncs:
            assert hit, f"{c.name} is declared syncs=True but covers no entry of SYNCING"
        else:
            assert hit <= set(SC.SOMETIMES_ASYNC), f"{c.name} is declared syncs=False but covers {sorted(hit)} of SYNCING"


def test_integration_md_names_every_syncing_entry():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^### Streams\n(.*?)(?=^#{2,3} |\Z)", text, flags=re.S | re.M)
    assert m, 'INTEGRATION.md has no "### Streams" section'
    section = m.group(1)
    missing = [n for n in SC.SYNCING if f"`{n.replace('Model.', 'model.')}`" not in section]
    assert not missing, f"INTEGRATION.md's Streams section does not name {missing}"


def test_host_only_entries_launch_nothing():
    """Nothing that takes a stream argument of the library may be excused as host-only."""
    import imageretrievalresearch_amd as M
    from imageretrievalresearch_amd.models import MI355Model
    owners = {"Whitening": M.Whitening, "PreparedGallery": M.PreparedGallery, "Model": MI355Model, "ShardedGallery": M.ShardedGallery}
    for name in SC.HOST_ONLY:
        owner, _, attr = name.rpartition(".")
        obj = getattr(owners[owner], attr) if owner else getattr(M, name)
        if inspect.isclass(obj):
            continue
        src = inspect.getsource(obj.fget if isinstance(obj, property) else obj)
        assert "stream_ptr(" not in src, f"{name} passes a stream to the library: it needs a case"


# ---------------------------------------------------------------------------------------------- leaves and comparison
class _Pair(NamedTuple):
    values: torch.Tensor
    indices: torch.Tensor


class _Obj:
    def __init__(self, m, n):
        self.matrix, self.n, self._hidden = m, n, object()


def _result():
    v = torch.tensor([[1.0, float("nan")], [-0.0, 3.5]])
    return {"pair": _Pair(v.clone(), torch.tensor([[3, 1], [2, 0]])), "obj": _Obj(v.double(), 7), "list": [v.half(), None, 2.5, "x"],
            "flag": True}


def test_leaf_paths():
    paths = [p for p, _ in H.leaves(_result())]
    assert paths == ["r['flag']", "r['list'][0]", "r['list'][1]", "r['list'][2]", "r['list'][3]", "r['obj'].matrix", "r['obj'].n",
                     "r['pair'].values", "r['pair'].indices"]
    with pytest.raises(TypeError):
        H.leaves({"s": {1, 2}})


def test_a_nan_equals_the_same_nan_and_minus_zero_differs_from_zero():
    assert H.differences(_result(), _result()) == []
    assert H.differences(H.to_host(H.clone_leaves(_result())), H.clone_leaves(_result())) == []
    a, b = _result(), _result()
    b["pair"].values[1, 0] = 0.0                                    # +0 for -0: equal as floats, not as bits
    assert torch.equal(a["pair"].values[1], b["pair"].values[1])
    diff = H.differences(a, b)
    assert len(diff) == 1 and diff[0].startswith("r['pair'].values: 1 of 4 elements differ, first at flat index 2")
    q = torch.tensor([float("nan")])
    other = q.view(torch.int32).add(1).view(torch.float32)          # another NaN payload
    assert H.differences(q, q.clone()) == [] and len(H.differences(q, other)) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.int64, torch.int32, torch.int8, torch.uint8])
def test_one_bit_is_reported_with_its_leaf_path(dtype):
    a = {"out": (torch.arange(24).reshape(2, 3, 4).to(dtype), torch.zeros((), dtype=dtype))}
    b = H.to_host(a)
    assert H.differences(a, b) == []
    flat = b["out"][0].reshape(-1).view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a["out"][0].element_size()])
    flat[17] ^= 1
    diff = H.differences(a, b)
    assert len(diff) == 1 and diff[0].startswith("r['out'][0]: 1 of 24 elements differ, first at flat index 17"), diff
    with pytest.raises(AssertionError, match=r"r\['out'\]\[0\]"):
        H.assert_same(a, b, "case")
    b["out"][1].view(flat.dtype).fill_(1)                            # a 0-dim leaf
    assert len(H.differences(a, b)) == 2


def test_shape_dtype_structure_and_scalar_mismatches_fail():
    t = torch.zeros(2, 3)
    assert "shape" in H.differences((t,), (t.reshape(3, 2),))[0]
    assert "dtype" in H.differences((t,), (t.int(),))[0]
    assert "leaf structure" in H.differences((t,), (t, t))[0]
    assert "leaf structure" in H.differences({"a": t}, {"b": t})[0]
    assert H.differences((t, 3), (t, 3)) == [] and H.differences((t, 3), (t, 4)) == ["r[1]: 3 != 4"]
    assert H.differences((1,), (1.0,)) == ["r[0]: 1 != 1.0"] and H.differences((True,), (1,)) != []
    assert H.differences((float("nan"),), (float("nan"),)) == []
    assert H.differences((t, None), (t, None)) == [] and H.differences((None,), (t,)) != []
    assert H.differences(torch.tensor([True, False]), torch.tensor([True, True])) != []
