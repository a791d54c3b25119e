"""The embed executor's launch plan, per-op table and traffic model against a recording of the commit before the plan
existed (tests/golden/launch_plan_parent.json, made by tests/golden/make_launch_plan_golden.py): the refactor that put one
resolved plan under the executor must launch, size and report exactly what the spread-out decisions did.  Host-only."""
import json
import os

import pytest

import launch_plan_cases as K
from imageretrievalresearch_amd import _lib, create_model

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan_parent.json")))
LISTS = GOLDEN["lists"]


def _mine(d, name):
    return {k: v for k, v in d.items() if k.startswith(name + "|")}


def test_how_codes_are_the_recorded_ones():
    assert GOLDEN["how"] == K.HOW


@pytest.mark.parametrize("name", K.MODELS)
def test_steps_and_arena_equal_the_parent(name):
    got = K.collect_plans(_lib.lib(), name)
    want = _mine(GOLDEN["plans"], name)
    assert sorted(got) == sorted(want)
    n_ops_model = len(LISTS[GOLDEN["profile_ops"][f"{name}|1|224x224"][1]])
    kinds_seen = set()
    for key, (first_op, n_ops, how, arena) in got.items():
        # every op index is covered by exactly one step, in order
        assert first_op[0] == 0 and all(n >= 1 for n in n_ops), key
        assert all(first_op[i + 1] == first_op[i] + n_ops[i] for i in range(len(n_ops) - 1)), key
        assert first_op[-1] + n_ops[-1] == n_ops_model, key
        steps, want_arena = want[key]
        assert (first_op, n_ops, how) == K.decode_steps(LISTS[steps]), key
        assert arena == want_arena, key
        kinds_seen.update(how)
    # the cases reach every way a step of this family can run
    assert kinds_seen == ({0, 6} if name.startswith("swin") else {0, 1, 2, 3, 4, 5}), kinds_seen


@pytest.mark.parametrize("name", K.MODELS)
def test_traffic_kinds_equal_the_parent(name):
    got = K.collect_traffic(_lib.lib(), name)
    want = _mine(GOLDEN["traffic"], name)
    assert sorted(got) == sorted(want)
    for key, v in got.items():
        assert v == LISTS[want[key]], key          # whole numbers far below 2^53: exact


@pytest.mark.parametrize("name", K.MODELS)
def test_profile_ops_equal_the_parent(name):
    got = K.collect_profile_ops(_lib.lib(), name)
    want = _mine(GOLDEN["profile_ops"], name)
    assert sorted(got) == sorted(want)
    for key, (labels, kinds, by) in got.items():
        wl, wk, wb = (LISTS[i] for i in want[key])
        assert labels == wl and kinds == wk and by == wb, key


def test_model_plan_binding():
    m = create_model("efficientnet_b3a", num_classes=0)
    steps, arena = m.plan(256, chunk=128)
    want, want_arena = GOLDEN["plans"]["efficientnet_b3a|256|128|224x224|defaults|pooled"]
    first_op, n_ops, how = K.decode_steps(LISTS[want])
    assert steps == list(zip(first_op, n_ops, (K.HOW[h] for h in how))) and arena == want_arena
    assert m.plan(256, chunk=128, pooled=False)[0][-1] == (first_op[-1], 1, "op")
    with pytest.raises(_lib.MI355Error, match="bad shape"):
        m.plan(4, chunk=5)
