"""Filtered against unfiltered search time (developer tool), fp32 and fp16 galleries, on the same synthetic rows and queries
(1000 classes; label_filter="same" plus a leave-one-out exclude, and the exclude alone).  The variants run in alternation, each rep timed with
HIP events around ``--calls`` back-to-back searches; the median of the reps is reported, one JSON line per case.  A last
line times ``retrieval_accuracy`` on a same-source set (``--acc``: rows x classes, R ~ rows / classes).

    python tools/bench_rank_filtered.py [--reps 15] [--calls 10] [--cases 256x100000x3,1x100000x3,256x100000x100]
                                        [--acc 100000x1000]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import synth  # noqa: E402

D = 1536


def _time(variants, reps, calls):
    for fn in variants.values():                         # warm-up (the first calls of a process run slower)
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / calls)
    return {name: statistics.median(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cases", default="256x100000x3,1x100000x3,256x100000x100")
    ap.add_argument("--acc", default="100000x1000")
    a = ap.parse_args()
    dev = "cuda:0"
    for case in a.cases.split(","):
        Q, G, k = (int(v) for v in case.split("x"))
        q = M.synth_fill(Q * D, 13, synth.NORMAL, dev).view(Q, D)
        x = M.synth_fill(G * D, 5, synth.NORMAL, dev).view(G, D)
        gl = torch.arange(G, device=dev) % 1000
        ql = torch.arange(Q, device=dev) % 1000
        ex = torch.arange(Q, device=dev) * 7
        g32 = M.Gallery(D, dev, capacity=G).add(x, gl)
        g16 = M.Gallery(D, dev, capacity=G, dtype=torch.float16).add(x, gl)
        del x
        variants = {}
        for name, g in (("fp32", g32), ("fp16", g16)):
            variants[name] = (lambda g=g: g.search(q, k))
            variants[name + "_filtered"] = (lambda g=g: g.search(q, k, query_labels=ql, label_filter="same", exclude=ex))
            # exclude only: as many rows are eligible (and inserted) as without the filter - the filter's own cost
            variants[name + "_exclude"] = (lambda g=g: g.search(q, k, exclude=ex))
        med = _time(variants, a.reps, a.calls)
        out = {"Q": Q, "G": G, "D": D, "k": k, "reps": a.reps, "calls": a.calls}
        for name, ms in med.items():
            out[f"{name}_ms"] = round(ms, 4)
        for name in ("fp32", "fp16"):
            out[f"{name}_filtered_ratio"] = round(med[name + "_filtered"] / med[name], 3)
            out[f"{name}_exclude_ratio"] = round(med[name + "_exclude"] / med[name], 3)
        print(json.dumps(out), flush=True)
        del g32, g16
        torch.cuda.empty_cache()
    if a.acc:
        n, classes = (int(v) for v in a.acc.split("x"))
        x = M.synth_fill(n * D, 7, synth.NORMAL, dev).view(n, D)
        lab = torch.arange(n, device=dev) % classes
        M.retrieval_accuracy(x[:2000], lab[:2000])          # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = M.retrieval_accuracy(x, lab)
            r["map_at_r"].item()
            ts.append(time.perf_counter() - t0)
        print(json.dumps({"retrieval_accuracy": f"{n}x{D}", "classes": classes, "R": int(r["R"].max()),
                          "seconds_median": round(statistics.median(ts), 3), "runs": len(ts)}), flush=True)


if __name__ == "__main__":
    main()
