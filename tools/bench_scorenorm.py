"""Score normalisation timings (developer tool).  One JSON line per (gallery dtype, rows); per number of queries Q, k = 3, in ms:

* ``search_normed``: ``Gallery.search_normed(q, k, norm)`` with a CSLS norm, split into ``query_side`` (the n = 10 search of the
  query's neighbourhood and its statistics) and ``adjusted`` (``adjusted_topk`` alone, with coefficient vectors made beforehand:
  the cosine GEMM with the map in front of the fused selection);
* ``search``: the plain ``Gallery.search(q, k)`` of the same commit, and ``adjusted_over_search`` = adjusted / search: what the
  epilogue's extra loads cost;
* ``torch``: what a user would write without the entries - the cosine slab (``cosine_scores``; for fp16 rows a half-precision
  ``matmul`` against the resident rows), the map in torch arithmetic, ``torch.topk`` - and ``adjusted_over_torch``.

All variants in alternation in one process, HIP events around ``--calls`` back-to-back calls, median of ``--reps`` after warm-up.
``fit_ms``: ``Gallery.score_norm(cohort, "csls")`` for the gallery against ``--cohort`` rows, host clock around a synchronised
call (it reads the finite check back).  Clustered synthetic rows, those of tools/bench_diversify.py.

    python tools/bench_scorenorm.py [--dtypes fp32 fp16] [--dim 1536] [--rows 100000 1000000] [--out profiles/scorenorm_bench.txt]
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
        for _ in range(2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", choices=("fp32", "fp16"), nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--queries", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--cohort", type=int, default=10000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scorenorm.py measures on the GPU: there is no CPU path"
    dev = "cuda:0"
    Dm, Qmax, Gmax = a.dim, max(a.queries), max(a.rows)
    gen = torch.Generator(device=dev).manual_seed(1)
    centers = torch.randn(1000, Dm, device=dev, generator=gen)
    lab = torch.randint(0, 1000, (Gmax + Qmax + a.cohort,), device=dev, generator=gen)
    x = centers[lab] + a.spread * torch.randn(Gmax + Qmax + a.cohort, Dm, device=dev, generator=gen)
    queries, cohort = x[Gmax: Gmax + Qmax], x[Gmax + Qmax:]
    for dtype in a.dtypes:
        for G in a.rows:
            gal = M.Gallery(Dm, dev, capacity=G, dtype=torch.float16 if dtype == "fp16" else torch.float32).add(x[:G])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            norm = gal.score_norm(cohort, "csls")
            torch.cuda.synchronize()
            fit_ms = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            norm = gal.score_norm(cohort, "csls")                    # (the second call: workspaces and code objects are warm)
            torch.cuda.synchronize()
            fit_warm_ms = round((time.perf_counter() - t0) * 1e3, 1)
            result = {}
            for Q in a.queries:
                q = queries[:Q].contiguous()
                aq, bq = norm.query_side(gal, q)

                def torch_way():
                    if dtype == "fp16":
                        S = (M.l2_normalize_rows(q).half() @ gal.data.T).float()
                    else:
                        S = M.cosine_scores(q, gal.data, gallery_is_normalized=True)
                    return torch.topk(S * aq[:, None] - (bq[:, None] + norm.bg[None, :]), a.k, dim=1)

                t = _time({"search_normed": lambda: gal.search_normed(q, a.k, norm), "query_side": lambda: norm.query_side(gal, q),
                           "adjusted": lambda: M.adjusted_topk(q, gal, a.k, aq=aq, bq=bq, bg=norm.bg),
                           "search": lambda: gal.search(q, a.k), "torch": torch_way}, a.reps, a.calls)
                t["adjusted_over_search"] = round(t["adjusted"] / t["search"], 3)
                t["adjusted_over_torch"] = round(t["adjusted"] / t["torch"], 3)
                t["normed_over_torch"] = round(t["search_normed"] / t["torch"], 3)
                got, ref = gal.search_normed(q, a.k, norm)[1], torch_way()[1]
                t["torch_top1_equal"] = round(float((got[:, 0] == ref[:, 0]).float().mean()), 4)
                result[f"Q{Q}"] = t
            line = json.dumps({"case": "scorenorm", "rows": G, "dim": Dm, "dtype": dtype, "k": a.k, "kind": "csls", "cohort": a.cohort,
                               "fit_ms": fit_ms, "fit_warm_ms": fit_warm_ms, "ms": result})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del gal, norm


if __name__ == "__main__":
    main()
