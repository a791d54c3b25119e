"""Diffusion re-ranking timings and quality (developer tool).  One JSON line per gallery dtype:

* ``graph_ms``: ``Gallery.knn_graph(kd)``, the blocked self-join, timed once; ``index_ms`` / ``index_bytes``: the rest of
  ``Gallery.diffusion_index(kd, gamma)`` (``mi355_diffusion_graph``) on that graph, timed once, and ``DiffusionIndex.nbytes``;
* per shortlist L: ``diffuse_ms`` (one ``Gallery.diffuse(q, 10, shortlist=L, iters=...)`` of 256 queries), ``search_ms`` (the plain
  ``search(q, L)``) and ``solve_ms`` (source vector + CG solve alone, on a shortlist made beforehand); ``rerank_ms`` is
  ``Gallery.rerank`` at its own shortlist.  All variants in alternation in one process, HIP events around ``--calls``
  back-to-back calls, median of ``--reps`` (after warm-up);
* quality against the class labels of the rows, the query's class being the relevant rows: ``p10`` (precision of the first 10)
  and ``rprec`` (the share of relevant rows among the first R results, R the class size cut to the list's length), for the plain
  search order, ``rerank`` and ``diffuse`` at each shortlist, every list as long as its shortlist.

Clustered synthetic rows (1000 classes), those of tools/rerank_timing.py.  Each dtype is one process:

    python tools/bench_diffusion.py [--dtype fp32] [--dim 1536] [--rows 100000] [--out profiles/diffusion_bench.txt]
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
from imageretrievalresearch_amd import diffusion as D  # noqa: E402
from imageretrievalresearch_amd import rerank as K  # noqa: E402


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
    return {name: round(statistics.median(v), 3) for name, v in times.items()}


def _once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round((time.perf_counter() - t) * 1e3, 2)


def _quality(idx, glab, qlab, sizes):
    """(p10, rprec) of ranked rows idx (Q, n): relevant = the rows of the query's class."""
    rel = (glab[idx.clamp_min(0)] == qlab[:, None]) & (idx >= 0)
    n = idx.shape[1]
    R = sizes[qlab].clamp(1, n)
    inside = torch.arange(n, device=idx.device)[None, :] < R[:, None]
    return (round(rel[:, :10].float().mean().item(), 4), round(((rel & inside).sum(1) / R).mean().item(), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtype", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--shortlists", type=int, nargs="+", default=[100, 200, 1024])
    ap.add_argument("--rerank-shortlist", type=int, default=100)
    ap.add_argument("--kd", type=int, default=20)
    ap.add_argument("--kq", type=int, default=10)
    ap.add_argument("--gamma", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=0.99)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_diffusion.py measures on the GPU: there is no CPU path"
    dev = "cuda:0"
    G, Q, Dm = a.rows, a.queries, a.dim
    gen = torch.Generator(device=dev).manual_seed(1)
    centers = torch.randn(1000, Dm, device=dev, generator=gen)
    lab = torch.randint(0, 1000, (G + Q,), device=dev, generator=gen)
    x = centers[lab] + a.spread * torch.randn(G + Q, Dm, device=dev, generator=gen)
    gal = M.Gallery(Dm, dev, dtype=torch.float16 if a.dtype == "fp16" else torch.float32).add(x[:G])
    q, glab, qlab = x[G:].contiguous(), lab[:G], lab[G:]
    sizes = torch.bincount(glab, minlength=1000)
    kw = dict(kd=a.kd, kq=a.kq, alpha=a.alpha, gamma=a.gamma, iters=a.iters)

    gal.search(q, a.kd, exclude=torch.arange(Q, device=dev))                     # warm-up of the search kernels
    _, graph_ms = _once(lambda: gal.knn_graph(a.kd))
    D._df_graph(*reversed(gal.knn_graph(a.kd)), a.gamma)                          # warm-up: the code object of the new kernels
    index, index_ms = _once(lambda: gal.diffusion_index(a.kd, a.gamma))
    gal.rerank_index()

    variants, lists = {}, {}
    for L in a.shortlists:
        sv, si = K._shortlist_search(gal, q, L, None)
        lists[L] = (sv.contiguous(), si.contiguous())
        variants[f"diffuse_ms@{L}"] = lambda L=L: gal.diffuse(q, 10, shortlist=L, **kw)
        variants[f"search_ms@{L}"] = lambda L=L: gal.search(q, L)
        variants[f"solve_ms@{L}"] = lambda L=L: D._df_solve(index.cols, index.vals, lists[L][1],
                                                             D._df_source(*lists[L], a.kq, a.gamma), a.alpha, a.iters)
    variants["rerank_ms"] = lambda: gal.rerank(q, 10, shortlist=a.rerank_shortlist)
    t = _time(variants, a.reps, a.calls)

    quality, iterations = {}, {}
    for L in a.shortlists:
        quality[f"search@{L}"] = _quality(gal.search(q, L)[1], glab, qlab, sizes)
        _, idx, its = gal.diffuse(q, L, shortlist=L, stats=True, **kw)
        quality[f"diffuse@{L}"] = _quality(idx, glab, qlab, sizes)
        iterations[str(L)] = [int(its.min()), int(its.max())]
    Lr = a.rerank_shortlist
    quality[f"rerank@{Lr}"] = _quality(gal.rerank(q, Lr, shortlist=Lr)[1], glab, qlab, sizes)
    line = json.dumps({"case": "diffusion", "rows": G, "dim": Dm, "dtype": a.dtype, "queries": Q, "spread": a.spread, **kw,
                       "graph_ms": graph_ms, "index_ms": index_ms, "index_bytes": index.nbytes,
                       "mutual_slots": round((index.cols >= 0).float().mean().item(), 4), "lds_bytes": {str(L): D.lds_bytes(L, a.kd)
                                                                                                     for L in a.shortlists},
                       **t, "iterations_min_max": iterations, "p10_rprec": quality})
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
