"""Full-gallery ranking timings (developer tool): ``ranking_metrics`` on a same-source set of ``--rows`` x 1536 fp32 rows in
``--classes`` classes, split into its three phases (positives, count, finalize), next to ``verification_roc`` on the same rows
(the same GEMM loop with the histogram epilogue: the floor the counting pass sits on) and ``retrieval_accuracy`` at the same
labels (the only other route to a MAP-type number).  The variants run in alternation, each rep timed with HIP events; the
median of the reps is reported as one JSON line, with the share of the negatives that beat their query's weakest positive
(each of those costs a binary search and an atomic).

    python tools/bench_ranking.py [--rows 100000] [--classes 1000] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import rank as R  # noqa: E402
from imageretrievalresearch_amd import synth  # noqa: E402

D = 1536


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    n = a.rows
    x = M.synth_fill(n * D, 7, synth.NORMAL, dev).view(n, D)
    lab = torch.arange(n, device=dev) % a.classes
    ex = torch.arange(n, device=dev)
    rows = R._Rows.of(x)
    times = {k: [] for k in ("positives", "count", "finalize", "ranking_metrics", "verification_roc", "retrieval_accuracy")}
    share = None
    for rep in range(a.reps + 1):                         # the first round is the warm-up
        tp, (off, keys, idx, sc) = _timed(lambda: R._ranks_positives(x, lab, rows, lab, ex, 0, 1e-6))
        tc, before = _timed(lambda: R._ranks_count(x, lab, rows, lab, ex, 0, 1e-6, off, keys))
        tf, _ = _timed(lambda: R._ranks_finalize(off, before))
        tm, m = _timed(lambda: M.ranking_metrics(x, lab))
        tr, _ = _timed(lambda: M.verification_roc(x, lab))
        ta, acc = _timed(lambda: M.retrieval_accuracy(x, lab))
        if rep == 0:
            negatives = n * (n - 1) - keys.numel()
            share = float(before.sum(dtype=torch.int64)) / negatives
            continue
        for k, v in zip(times, (tp, tc, tf, tm, tr, ta)):
            times[k].append(v)
    out = {"rows": n, "D": D, "classes": a.classes, "reps": a.reps, "positives": int(keys.numel()),
           "negatives_beating_weakest_positive": round(share, 4), "map": float(m["map"]), "map_at_r": float(acc["map_at_r"])}
    out.update({f"{k}_ms": round(statistics.median(v), 2) for k, v in times.items()})
    out["count_over_roc"] = round(out["count_ms"] / out["verification_roc_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
