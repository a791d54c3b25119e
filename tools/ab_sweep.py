"""Developer tool: A/B two builds of the library on the row-sweep launches, alternated on one GPU in one call.

    python tools/ab_sweep.py --parent /path/libparent.so [--new /path/libnew.so] [--rounds 5] [--stamps]

Each round starts one fresh process per arm - parent, new, parent again ("parent2": the parent against itself gives the
run-to-run spread) - with MI355_LIB_PATH pointing at that arm's library.  A process takes three samples of
  * the seven sweep launches of the EfficientNet-B3a forward at B = 256 from the executor's per-op profile (5 forwards each),
  * the whole forward of efficientnet_b3a, rexnet_150 and rexnet_200 at B = 256 (HIP events round 10 forwards),
so --rounds 5 gives 15 samples per arm; medians are reported, one JSON line at the end.  --stamps adds the wave-0 phase stamps of
the sweep launches (tools/tune_sweep.py's table) for the parent and the new build."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_OPS = (7, 11, 15, 19, 23, 27, 31)
B = 256


def child(stamps):
    sys.path.insert(0, ROOT)
    import torch
    import imageretrievalresearch_amd as M
    from imageretrievalresearch_amd import synth
    from oracle import effnet
    dev = "cuda:0"
    x = M.synth_fill(B * 3 * 224 * 224, 1, synth.UNIFORM, dev).view(B, 3, 224, 224)
    out = {"ops": {}, "sum": [], "fwd": {}}
    for name in ("efficientnet_b3a", "rexnet_150", "rexnet_200"):
        model = M.create_model(name, num_classes=0).to(dev).eval()
        if name == "efficientnet_b3a":
            model.load_state_dict(effnet.init_state_dict(2), strict=False)
        for _ in range(5):
            model(x)
        torch.cuda.synchronize()
        out["fwd"][name] = []
        for _ in range(3):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(10):
                model(x)
            t1.record()
            t1.synchronize()
            out["fwd"][name].append(t0.elapsed_time(t1) / 10)
        if name != "efficientnet_b3a":
            continue
        for _ in range(3):
            model.set_option("profile", 1)
            for _ in range(5):
                model(x)
            model.profile_read()
            rows = model.profile_ops(B)
            model.set_option("profile", 0)
            for i in SWEEP_OPS:
                out["ops"].setdefault(f"{i} {rows[i][0]}", []).append(rows[i][2] * 1e3)
            out["sum"].append(sum(rows[i][2] for i in SWEEP_OPS) * 1e3)
        if stamps:
            model.set_option("block_stamps", 1)
            model(x)
            torch.cuda.synchronize()
            rows = model.profile_ops(B)
            out["stamps"] = {f"{i} {rows[i][0]}": [c / 1e3 for c in v[:10]] for i, v in model.block_stamps() if i in SWEEP_OPS}
            model.set_option("block_stamps", 0)
    print("AB_JSON " + json.dumps(out), flush=True)


def run_arm(lib, stamps):
    env = dict(os.environ)
    if lib:
        env["MI355_LIB_PATH"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--stamps"] if stamps else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"arm {lib} ended with status {p.returncode}")       # nothing more is started on the GPU
    line = [l for l in p.stdout.splitlines() if l.startswith("AB_JSON ")][-1]
    return json.loads(line[8:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--new", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.stamps)
    arms = {"parent": a.parent, "new": a.new, "parent2": a.parent}
    acc = {k: {"ops": {}, "sum": [], "fwd": {}} for k in arms}
    stamps = {}
    for r in range(a.rounds):
        for arm, lib in arms.items():
            want = a.stamps and r == 0 and arm != "parent2"
            o = run_arm(lib, want)
            acc[arm]["sum"] += o["sum"]
            for k, v in o["ops"].items():
                acc[arm]["ops"].setdefault(k, []).extend(v)
            for k, v in o["fwd"].items():
                acc[arm]["fwd"].setdefault(k, []).extend(v)
            if want:
                stamps[arm] = o["stamps"]
        print(f"round {r}: sweep sum us " + "  ".join(f"{k} {statistics.median(acc[k]['sum']):.1f}" for k in arms), flush=True)
    med = statistics.median
    print(f"\nper-op medians, us ({3 * a.rounds} samples per arm)            parent   parent2      new   new-parent   |parent2-parent|")
    for k in acc["parent"]["ops"]:
        p, q, n = (med(acc[arm]["ops"][k]) for arm in ("parent", "parent2", "new"))
        print(f"{k:44s} {p:8.1f} {q:8.1f} {n:8.1f} {n - p:+10.1f} {abs(q - p):10.1f}")
    p, q, n = (med(acc[arm]["sum"]) for arm in ("parent", "parent2", "new"))
    print(f"{'sum of the seven sweep launches':44s} {p:8.1f} {q:8.1f} {n:8.1f} {n - p:+10.1f} {abs(q - p):10.1f}")
    print("\nwhole forward at B = 256, ms                    parent   parent2      new")
    for k in acc["parent"]["fwd"]:
        print(f"{k:44s} " + " ".join(f"{med(acc[arm]['fwd'][k]):8.3f}" for arm in ("parent", "parent2", "new")))
    for arm, st in stamps.items():
        print(f"\n{arm}: kcycles summed over an image's workgroups (wave 0): init | slabconst | halo | xissue | xwait | expand | bar | dw | - | squeeze")
        for k, v in st.items():
            print(f"{k:32s} " + " ".join(f"{c:8.1f}" for c in v) + f" | {sum(v):8.1f}")
    print(json.dumps({arm: {"sweep_sum_us": med(acc[arm]["sum"]), "fwd_ms": {k: med(v) for k, v in acc[arm]["fwd"].items()}} for arm in arms}))


if __name__ == "__main__":
    main()
