"""IVF search timings (developer tool) on one MI355X: ``IVFIndex.search`` beside the exhaustive ``Gallery.search`` of the same
resident gallery in the same process, for fp32 and fp16 rows.

The gallery is a seeded mixture: ``--nlist`` planted unit centres, every row its centre plus Gaussian noise of the same length
(cosine to the own centre ~0.7), the queries drawn the same way.  Plain Gaussian rows have no lists worth probing.

Per (rows, dtype): the one-time costs (k-means + CSR build time, ``index.nbytes``), then for Q in {1, 256} and nprobe in
{1, 8, 32} at k = 3 one JSON line with

  exhaustive_ms .. ``Gallery.search(q, k)``
  ivf_ms ......... ``index.search(q, k, nprobe)``: probe, scan, merge, pads, and the scan's flag read
  scan_ms ........ the scan entry alone (``mi355_ivf_scan`` with the probes given)
  recall_at_k .... the share of the exhaustive top-k that the IVF search returns
  row_bytes ...... bytes of gallery rows the scan reads (every list once per group of up to 4 of its queries)
  scan_gbps ...... row_bytes / scan_ms

The variants run in alternation, each repetition timed with HIP events after a warm-up round; medians are reported.

    python tools/bench_ivf.py [--rows 100000 1000000] [--dim 1536] [--nlist 1024] [--reps 7] [--out profiles/ivf_bench.txt]
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
    """n rows: row i = centre ((first + i) mod nlist) + noise whose expected length is 1 (the centres are unit rows)."""
    K, D = centres.shape
    lab = (torch.arange(n, device=DEV) + first) % K
    noise = M.synth_fill(n * D, seed, synth.NORMAL, DEV).view(n, D) * (D ** -0.5)
    return centres[lab] + noise


def _row_bytes(index, probes, group=4):
    """Bytes of rows one scan streams: every list once per group of up to ``group`` of the queries that probe it."""
    pairs = torch.bincount(probes.reshape(-1), minlength=index.nlist)
    groups = (pairs + group - 1) // group
    g = index.gallery
    return int((groups * index.counts).sum()) * g._ld * g._buf.element_size()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ivf.py measures on the GPU; there is none here")
    D, K, k = a.dim, a.nlist, a.k
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        lines.append(line)
        print(line, flush=True)

    centres = M.l2_normalize_rows(M.synth_fill(K * D, 5, synth.NORMAL, DEV).view(K, D))
    queries = _mixture(256, centres, 9)
    for n in a.rows:
        for dtype in (torch.float32, torch.float16):
            g = M.Gallery(D, DEV, capacity=n, dtype=dtype)
            for r0 in range(0, n, PIECE):
                m = min(PIECE, n - r0)
                g.add(_mixture(m, centres, 100 + r0 // PIECE, first=r0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index = M.IVFIndex.build(g, K, iters=a.iters, seed=0)
            torch.cuda.synchronize()
            build_s = time.perf_counter() - t0
            counts = index.counts.cpu()
            emit({"rows": n, "D": D, "gallery": str(dtype).replace("torch.", ""), "nlist": K, "kmeans_iters": a.iters,
                  "build_s": round(build_s, 3), "index_bytes": index.nbytes, "gallery_bytes": g.nbytes,
                  "list_rows_min": int(counts.min()), "list_rows_median": int(counts.median()), "list_rows_max": int(counts.max())})
            for Q in (1, 256):
                q = queries[:Q].contiguous()
                for nprobe in (1, 8, 32):
                    probes = index.probe(q, nprobe)
                    cap = max(int(index._longest[nprobe]), k)
                    t = {"exhaustive": [], "ivf": [], "scan": []}
                    for rep in range(a.reps + 1):                  # the first round is the warm-up
                        te, (_, ei) = _timed(lambda: g.search(q, k))
                        ti, (_, ii) = _timed(lambda: index.search(q, k, nprobe))
                        ts, _ = _timed(lambda: index._scan(q, probes, cap, 0, None))
                        if rep:
                            for key, v in zip(t, (te, ti, ts)):
                                t[key].append(v)
                    rec = {"rows": n, "D": D, "gallery": str(dtype).replace("torch.", ""), "nlist": K, "Q": Q, "nprobe": nprobe,
                           "k": k, "reps": a.reps, "cap": cap}
                    rec.update({f"{key}_ms": round(statistics.median(v), 4) for key, v in t.items()})
                    rec["speedup"] = round(rec["exhaustive_ms"] / rec["ivf_ms"], 2)
                    rec["recall_at_k"] = round(float((ii.unsqueeze(2) == ei.unsqueeze(1)).any(1).double().mean()), 4)
                    rec["row_bytes"] = _row_bytes(index, probes)
                    rec["gallery_row_bytes"] = n * g._ld * g._buf.element_size()
                    rec["scan_gbps"] = round(rec["row_bytes"] / rec["scan_ms"] * 1e-6, 1)
                    emit(rec)
            del index, g
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_ivf.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
