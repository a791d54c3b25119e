"""Spherical k-means timings (developer tool): one ``assign_clusters``, one ``update_centroids`` and one full iteration on
``--rows`` x ``--dim`` rows with ``--clusters`` centroids, for a resident fp32 and a resident fp16 ``Gallery``, beside two baselines
measured in the same run:

  (a) ``cosine_topk(rows, centroids, 1)``: the rows as queries, the only route to assignments without the nearest epilogue;
  (b) the torch restatement: fp32 ``x @ c.T`` + ``argmax`` for the assignment, ``index_add_`` + normalise for the update
      (float atomics: its bits change from run to run).

The variants run in alternation, each rep timed with HIP events; the median of the reps is reported, one JSON line per dtype.

    python tools/bench_kmeans.py [--rows 100000] [--dim 1536] [--clusters 1000] [--reps 5]

``--dim`` not a multiple of 4 (70, say) takes the GEMM's exact-fp32 loop, where the nearest epilogue holds 2 waves per SIMD
against the search epilogue's 3 (profiles/kmeans_kernel_resources.txt).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import synth  # noqa: E402

def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def _torch_assign(xn, c):
    s = xn @ torch.nn.functional.normalize(c, dim=1).T
    return s.argmax(dim=1)


def _torch_update(xn, a, K, prev):
    s = torch.zeros((K, xn.shape[1]), dtype=torch.float32, device=xn.device).index_add_(0, a, xn)
    n = s.norm(dim=1, keepdim=True)
    return torch.where(n > 1e-6, s / n.clamp_min(1e-6), prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev, n, K, D = "cuda:0", a.rows, a.clusters, a.dim
    x = M.synth_fill(n * D, 7, synth.NORMAL, dev).view(n, D)
    c = x[:: n // K][:K].contiguous()
    for dtype in (torch.float32, torch.float16):
        g = M.Gallery(D, dev, capacity=n, dtype=dtype).add(x)
        xn = g.data.float().contiguous()                  # baseline (b) and the queries of baseline (a): normalised fp32 rows
        times = {k: [] for k in ("assign", "update", "iteration", "topk1_assign", "torch_assign", "torch_update")}
        agree = None
        for rep in range(a.reps + 1):                     # the first round is the warm-up
            ta, (asg, _) = _timed(lambda: M.assign_clusters(g, c))
            tu, _ = _timed(lambda: M.update_centroids(g, asg, K, c))
            ti, _ = _timed(lambda: M.update_centroids(g, M.assign_clusters(g, c)[0], K, c))
            tk, (_, idx) = _timed(lambda: M.cosine_topk(xn, c, 1))
            tta, targ = _timed(lambda: _torch_assign(xn, c))
            ttu, _ = _timed(lambda: _torch_update(xn, asg, K, c))
            if rep == 0:
                agree = (float((idx[:, 0] == asg).float().mean()), float((targ == asg).float().mean()))
                continue
            for k, v in zip(times, (ta, tu, ti, tk, tta, ttu)):
                times[k].append(v)
        out = {"rows": n, "D": D, "clusters": K, "gallery": str(dtype).replace("torch.", ""), "reps": a.reps,
               "agree_with_topk1": round(agree[0], 6), "agree_with_torch": round(agree[1], 6)}
        out.update({f"{k}_ms": round(statistics.median(v), 3) for k, v in times.items()})
        out["assign_tflops"] = round(2.0 * n * K * D / out["assign_ms"] * 1e-9, 1)
        out["update_gbps"] = round(n * D * (4 if dtype == torch.float32 else 2) / out["update_ms"] * 1e-6, 1)
        print(json.dumps(out), flush=True)
        del g, xn


if __name__ == "__main__":
    main()
