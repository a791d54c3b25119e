"""Graph search timings (developer tool) on one MI355X: ``GraphIndex.search`` beside ``IVFIndex.search`` and the exhaustive
``Gallery.search`` of the same resident gallery in the same process, for fp32 and fp16 rows.

The gallery is the seeded mixture of tools/bench_ivf.py: ``--nlist`` planted unit centres, every row its centre plus Gaussian
noise of the same length, the queries drawn the same way.

Per (rows, dtype): the one-time costs (IVF build; the graph build - exact kNN graph, merge, k-means, entry points - and
``index.nbytes`` of both), then for Q in {1, 256} at k = 3 one JSON line with

  exhaustive_ms .. ``Gallery.search(q, k)``
  ivf ............ per nprobe in {1, 8, 32}: ``ivf_ms`` of ``IVFIndex.search(q, k, nprobe)``, its recall and the row bytes it scans
  graph .......... per ef in {16, 64, 128} (nseed 8): ``graph_ms`` of ``GraphIndex.search(q, k, ef, nseed)`` (seeds, walk and the
                   flag read), ``walk_ms`` with the seeds given, its recall, the mean ``iters`` and ``visited`` per query and the
                   row bytes read (visited x ld x element size)

Recall is the share of the exhaustive top-k returned.  The variants run in alternation, each repetition timed with HIP events
after a warm-up round; medians are reported.

    python tools/bench_graph.py [--rows 100000 1000000] [--dim 1536] [--nlist 1024] [--degree 32] [--reps 7]
                                [--out profiles/graph_bench.txt]
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
from bench_ivf import DEV, PIECE, _mixture, _row_bytes, _timed  # noqa: E402
from imageretrievalresearch_amd import synth  # noqa: E402

NPROBES, EFS, NSEED = (1, 8, 32), (16, 64, 128), 8


def _recall(got, want):
    return round(float((got.unsqueeze(2) == want.unsqueeze(1)).any(1).double().mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_graph.py measures on the GPU; there is none here")
    D, K, k = a.dim, a.nlist, a.k
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        lines.append(line)
        print(line, flush=True)

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write("# tools/bench_graph.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")

    centres = M.l2_normalize_rows(M.synth_fill(K * D, 5, synth.NORMAL, DEV).view(K, D))
    queries = _mixture(256, centres, 9)
    for n in a.rows:
        for dtype in (torch.float32, torch.float16):
            name = str(dtype).replace("torch.", "")
            g = M.Gallery(D, DEV, capacity=n, dtype=dtype)
            for r0 in range(0, n, PIECE):
                m = min(PIECE, n - r0)
                g.add(_mixture(m, centres, 100 + r0 // PIECE, first=r0))
            esz = g._ld * g._buf.element_size()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ivf = M.IVFIndex.build(g, K, iters=a.iters, seed=0)
            torch.cuda.synchronize()
            ivf_build_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            fwd = g.knn_graph(a.degree // 2)[1]
            torch.cuda.synchronize()
            knn_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            gi = M.GraphIndex.build(g, K, degree=a.degree, iters=a.iters, seed=0)     # the kNN graph is cached by the gallery
            torch.cuda.synchronize()
            rest_s = time.perf_counter() - t0
            pads = float((gi.graph < 0).double().mean())
            emit({"rows": n, "D": D, "gallery": name, "nlist": K, "nentry": K, "degree": a.degree, "kmeans_iters": a.iters,
                  "ivf_build_s": round(ivf_build_s, 3), "ivf_bytes": ivf.nbytes, "graph_knn_s": round(knn_s, 3),
                  "graph_merge_kmeans_entries_s": round(rest_s, 3), "graph_build_s": round(knn_s + rest_s, 3),
                  "graph_bytes": gi.nbytes, "graph_pad_share": round(pads, 4), "gallery_bytes": g.nbytes})
            del fwd
            for Q in (1, 256):
                q = queries[:Q].contiguous()
                seeds = gi.seeds(q, NSEED)
                t = {"exhaustive": []}
                t.update({f"ivf{p}": [] for p in NPROBES})
                t.update({f"graph{e}": [] for e in EFS})
                t.update({f"walk{e}": [] for e in EFS})
                last = {}
                for rep in range(a.reps + 1):                      # the first round is the warm-up
                    ms, last["exhaustive"] = _timed(lambda: g.search(q, k))
                    if rep:
                        t["exhaustive"].append(ms)
                    for p in NPROBES:
                        ms, last[f"ivf{p}"] = _timed(lambda: ivf.search(q, k, p))
                        if rep:
                            t[f"ivf{p}"].append(ms)
                    for e in EFS:
                        ms, last[f"graph{e}"] = _timed(lambda: gi.search(q, k, e, NSEED, stats=True))
                        ms2, _ = _timed(lambda: gi.search(q, k, e, seeds=seeds))
                        if rep:
                            t[f"graph{e}"].append(ms)
                            t[f"walk{e}"].append(ms2)
                med = {key: round(statistics.median(v), 4) for key, v in t.items()}
                want = last["exhaustive"][1]
                rec = {"rows": n, "D": D, "gallery": name, "Q": Q, "k": k, "reps": a.reps, "exhaustive_ms": med["exhaustive"],
                       "gallery_row_bytes": n * esz, "ivf": [], "graph": []}
                for p in NPROBES:
                    rec["ivf"].append({"nprobe": p, "ivf_ms": med[f"ivf{p}"], "recall_at_k": _recall(last[f"ivf{p}"][1], want),
                                       "row_bytes": _row_bytes(ivf, ivf.probe(q, p))})
                for e in EFS:
                    _, gi_idx, iters, visited = last[f"graph{e}"]
                    rec["graph"].append({"ef": e, "nseed": NSEED, "graph_ms": med[f"graph{e}"], "walk_ms": med[f"walk{e}"],
                                         "recall_at_k": _recall(gi_idx, want), "iters_mean": round(float(iters.double().mean()), 2),
                                         "visited_mean": round(float(visited.double().mean()), 1),
                                         "row_bytes": int(visited.sum()) * esz})
                emit(rec)
                flush()
            del ivf, gi, g
            torch.cuda.empty_cache()
    flush()


if __name__ == "__main__":
    main()
