"""DBSCAN timings (developer tool) on one MI355X: ``dbscan`` of a resident gallery, phase by phase, beside what a user had
before it, in the same process, for fp32 and fp16 rows.

The gallery is the seeded mixture of tools/bench_ivf.py: ``--clusters`` planted unit centres, every row its centre plus Gaussian
noise of the same length (cosine of two rows of one centre ~0.5, of two centres ~0).  The threshold is the midpoint between the
median score of same-centre pairs and the median score of different-centre pairs of a 256-row sample against all rows (the
planted labels are used for this choice and for the scores below, never by the clustering).

Per (rows, dtype) one JSON line with

  degree_ms, link_ms, finish_ms, dbscan_ms .. pass 1, pass 2, the finishing kernel + dense numbering, and one whole ``dbscan``
  roc_sweep_ms ........ one ``Gallery.verification_roc`` self-join of the same rows: one GEMM sweep with a counting epilogue
  range_count_ms ...... one count-only sweep of the range epilogue (``mi355_cosine_range`` with capacity 0) in the same blocks:
                        what pass 1 would cost on ``RangeArgs``
  range_ms, host_cc_ms  ``range_search`` of the gallery against itself (nnz pairs, csr_bytes) and the connected components of
                        that CSR on the host (copy to the host + scipy ``connected_components``)
  nmi / purity / f1 ... of ``dbscan`` labels, and of ``spherical_kmeans(K = clusters)`` assignments, against the planted centres

The variants run in alternation, each repetition timed with HIP events (a host clock for the host part) after a warm-up round;
medians are reported.

    python tools/dbscan_bench.py [--rows 100000 10000] [--dim 1536] [--clusters 1000] [--reps 5] [--out profiles/dbscan_bench.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import cluster, rank, synth  # noqa: E402
from imageretrievalresearch_amd._lib import check, lib, stream_ptr  # noqa: E402

DEV = "cuda:0"
PIECE = 50000                       # rows generated and added at a time


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def _mixture(n, centres, seed, first=0):
    K, D = centres.shape
    lab = (torch.arange(n, device=DEV) + first) % K
    noise = M.synth_fill(n * D, seed, synth.NORMAL, DEV).view(n, D) * (D ** -0.5)
    return centres[lab] + noise, lab


def _threshold(g, labels, sample=256):
    s = M.cosine_scores(g.data[:sample], g.data, gallery_is_normalized=True)
    same = labels[:sample, None] == labels[None, :]
    same[torch.arange(sample), torch.arange(sample)] = False            # not the row itself
    other = labels[:sample, None] != labels[None, :]
    lo, hi = float(s[other].median()), float(s[same].median())
    return 0.5 * (lo + hi), lo, hi


def _range_count_only(g, t, block):
    """The range epilogue in its count-only mode over the self-join, a block of rows per call; returns the hits."""
    L, src = lib(), g._resident()
    entry, ws_bytes = rank._ENTRIES[src.dtype]["range"]
    ws = rank._ws.get(DEV, getattr(L, ws_bytes)(block, src.rows, src.dim))
    nnz, total = ctypes.c_int64(0), 0
    for q0 in range(0, src.rows, block):
        q = src.data[q0: q0 + block].float().contiguous()
        check(getattr(L, entry)(q.data_ptr(), q.shape[0], *src.c_args(), g.eps, t, 0, None, None, 0, ctypes.byref(nnz),
                                ws.data_ptr(), ws.numel(), stream_ptr(DEV)))
        total += int(nnz.value)
    return total


def _host_components(r, n):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    offsets, indices = r.offsets.cpu().numpy(), r.indices.cpu().numpy()
    graph = csr_matrix((np.ones(len(indices), dtype=np.int8), indices, offsets), shape=(n, n))
    count, labels = connected_components(graph, directed=True, connection="weak")
    return (time.perf_counter() - t0) * 1e3, count, labels


def _scores(assign, planted):
    m = M.clustering_metrics(assign, planted)
    return {k: round(m[k], 4) for k in ("nmi", "purity", "f1")} | {"n_clusters": m["n_clusters"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dbscan_bench.py measures on the GPU; there is none here")
    D, K, ms = a.dim, a.clusters, a.min_samples
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        lines.append(line)
        print(line, flush=True)

    centres = M.l2_normalize_rows(M.synth_fill(K * D, 5, synth.NORMAL, DEV).view(K, D))
    for n in a.rows:
        for dtype in (torch.float32, torch.float16):
            g = M.Gallery(D, DEV, capacity=n, dtype=dtype)
            for r0 in range(0, n, PIECE):
                x, lab = _mixture(min(PIECE, n - r0), centres, 100 + r0 // PIECE, first=r0)
                g.add(x, lab)
            del x
            planted = g.labels.long()
            t, lo, hi = _threshold(g, planted)
            block = min(cluster._DBSCAN_BLOCK if a.block is None else a.block, n)
            allq = g.data.float() if dtype == torch.float16 else g.data          # the fp32 queries of the older routes
            times = {k: [] for k in ("degree", "link", "finish", "dbscan", "roc_sweep", "range_count", "range", "host_cc")}
            for rep in range(a.reps + 1):                                         # the first round is the warm-up
                run = cluster._DBSCANRun(g._resident(), t, ms, block, g.eps)
                td, _ = _timed(lambda: run.sweep(False))
                tl, _ = _timed(lambda: run.sweep(True))
                tf, res = _timed(run.finish)
                tw, whole = _timed(lambda: g.dbscan(t, ms, block=block))
                tr, _ = _timed(lambda: g.verification_roc(allq, planted))
                tc, counted = _timed(lambda: _range_count_only(g, t, block))
                tg, r = _timed(lambda: g.range_search(allq, t))
                th, ncomp, host_labels = _host_components(r, n)
                if rep:
                    for key, v in zip(times, (td, tl, tf, tw, tr, tc, tg, th)):
                        times[key].append(v)
            nnz = int(r.offsets[-1])
            assert counted == nnz == int(res.degree.sum()), (counted, nnz, int(res.degree.sum()))
            assert all(torch.equal(getattr(res, f), getattr(whole, f)) for f in ("labels", "core", "degree", "roots", "counts"))
            comp = g.components(t, block=block)                                   # the GPU's components against the host's
            same_partition = len(set(zip(comp.labels.tolist(), host_labels.tolist()))) == comp.n_clusters == ncomp
            km = g.kmeans(K, iters=20, seed=0)
            rec = {"rows": n, "D": D, "gallery": str(dtype).replace("torch.", ""), "clusters": K, "min_samples": ms, "block": block,
                   "threshold": round(t, 4), "median_other_centre": round(lo, 4), "median_same_centre": round(hi, 4), "reps": a.reps}
            rec.update({f"{key}_ms": round(statistics.median(v), 3) for key, v in times.items()})
            rec["dbscan_over_roc_sweep"] = round(rec["dbscan_ms"] / rec["roc_sweep_ms"], 2)
            rec["link_over_degree"] = round(rec["link_ms"] / rec["degree_ms"], 2)
            rec["degree_over_range_count"] = round(rec["degree_ms"] / rec["range_count_ms"], 2)
            rec["range_plus_host_over_dbscan"] = round((rec["range_ms"] + rec["host_cc_ms"]) / rec["dbscan_ms"], 2)
            rec.update({"nnz": nnz, "csr_bytes": nnz * 12 + (n + 1) * 8, "components_match_host": bool(same_partition),
                        "dbscan_clusters": res.n_clusters, "dbscan_noise": res.n_noise, "core_rows": int(res.core.sum()),
                        "dbscan": _scores(res.labels, planted), "kmeans": _scores(km.assignments, planted),
                        "kmeans_iterations": km.iterations, "dbscan_vs_kmeans": _scores(res.labels, km.assignments)})
            emit(rec)
            del g, allq, r, res, whole, comp, km, run
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/dbscan_bench.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
