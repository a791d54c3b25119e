"""Records tests/golden/launch_plan_parent.json: what the executor of the commit BEFORE the launch plan launched, sized
and reported, for every case of tests/launch_plan_cases.py.  Host-only (no GPU).

    python tests/golden/make_launch_plan_golden.py --lib PARENT.so --plan-lib PARENT_WITH_PLAN_ENTRY.so [--write]

--lib       the parent commit's library, unmodified: mi355_model_traffic_kinds and mi355_model_profile_ops come from it.
--plan-lib  the parent commit built with a recording-only mi355_model_plan on top of its own plan_slots, can_fuse_block,
            can_fuse, fused_late_supported, use_sweep, fused_band_rows, head conditions and LayerNorm-fold condition
            (a walk in the style of its traffic_kinds); steps and arena bytes come from it.
Without --write the result is compared with the committed file and nothing is written.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import launch_plan_cases as K  # noqa: E402

OUT = os.path.join(HERE, "launch_plan_parent.json")


def record(lib, plan_lib):
    lists, index = [], {}

    def intern(v):
        k = json.dumps(v)
        if k not in index:
            index[k] = len(lists)
            lists.append(v)
        return index[k]

    g = {"how": K.HOW, "lists": lists, "plans": {}, "traffic": {}, "profile_ops": {}}
    for name in K.MODELS:
        for key, (fo, no, hw, arena) in K.collect_plans(plan_lib, name).items():
            g["plans"][key] = [intern(K.encode_steps(fo, no, hw)), arena]
        for key, v in K.collect_traffic(lib, name).items():
            g["traffic"][key] = intern(v)
        for key, (labels, kinds, by) in K.collect_profile_ops(lib, name).items():
            g["profile_ops"][key] = [intern(labels), intern(kinds), intern(by)]
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--plan-lib", required=True)
    ap.add_argument("--write", action="store_true", help="overwrite the committed golden file")
    a = ap.parse_args()
    g = record(K.bind(ctypes.CDLL(a.lib), plan=False), K.bind(ctypes.CDLL(a.plan_lib)))
    text = json.dumps(g, separators=(",", ":"), sort_keys=True) + "\n"
    if os.path.exists(OUT) and not a.write:
        same = open(OUT).read() == text
        print("recording", "equals" if same else "DIFFERS from", OUT, "(not written; pass --write to overwrite)")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote", OUT, len(text), "bytes;", len(g["plans"]), "plans,", len(g["traffic"]), "traffic tables,",
          len(g["profile_ops"]), "per-op tables,", len(g["lists"]), "distinct lists")


if __name__ == "__main__":
    main()
