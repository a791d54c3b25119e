"""k-reciprocal re-ranking timings (developer tool).  One JSON line per (dim, gallery dtype):

* ``graph_ms``: ``Gallery.knn_graph(k1)``, the blocked self-join (``search(..., exclude=arange)``), timed once;
* ``index_ms`` / ``index_bytes``: the rest of ``Gallery.rerank_index(k1, k2)`` (sets, weights, local expansion of every gallery
  row) on that graph, timed once, and ``RerankIndex.nbytes``;
* ``rerank_ms``: one ``Gallery.rerank`` of 256 queries at shortlist K, next to ``search_ms``, the plain ``search(q, K)`` of the
  same process; both in alternation, HIP events around ``--calls`` back-to-back calls, median of ``--reps`` (after warm-up).

Clustered synthetic data (1000 classes), so that reciprocal sets are not trivial.  Each (dim, dtype) is one process:

    python tools/rerank_timing.py --dim 1536 [--dtype fp32] [--rows 100000] [--shortlist 100] [--out profiles/FILE]
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


def _time(variants, reps, calls):
    for fn in variants.values():
        for _ in range(3):
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


def _once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtype", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--shortlist", type=int, default=100)
    ap.add_argument("--k1", type=int, default=20)
    ap.add_argument("--k2", type=int, default=6)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    G, Q, D = a.rows, a.queries, a.dim
    gen = torch.Generator(device=dev).manual_seed(1)
    centers = torch.randn(1000, D, device=dev, generator=gen)
    lab = torch.randint(0, 1000, (G + Q,), device=dev, generator=gen)
    x = centers[lab] + 2.0 * torch.randn(G + Q, D, device=dev, generator=gen)
    gal = M.Gallery(D, dev, dtype=torch.float16 if a.dtype == "fp16" else torch.float32).add(x[:G])
    q = x[G:].contiguous()
    gal.search(q, a.k1, exclude=torch.arange(Q, device=dev))                     # warm-up of the search kernels
    _, graph_ms = _once(lambda: gal.knn_graph(a.k1))
    index, index_ms = _once(lambda: gal.rerank_index(a.k1, a.k2))
    t = _time({"rerank": lambda: gal.rerank(q, 10, k1=a.k1, k2=a.k2, shortlist=a.shortlist),
               "search": lambda: gal.search(q, a.shortlist)}, a.reps, a.calls)
    line = json.dumps({"case": "rerank", "rows": G, "dim": D, "dtype": a.dtype, "queries": Q, "k1": a.k1, "k2": a.k2,
                       "shortlist": a.shortlist, "graph_ms": round(graph_ms, 2), "index_ms": round(index_ms, 2),
                       "index_bytes": index.nbytes, "index_nnz_V": index.V.cols.numel(), "index_nnz_V2": index.V2.cols.numel(),
                       "rerank_ms": round(t["rerank"], 3), "search_ms": round(t["search"], 3)})
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
