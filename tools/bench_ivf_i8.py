"""Int8 IVF search timings (developer tool) on one MI355X: ``Int8IVFIndex.search`` and its scan beside ``IVFIndex`` over the
fp16 and the fp32 gallery ON THE SAME LISTS, the exhaustive ``Int8Gallery.search``, and the refined int8 search, all in one
process.

The gallery is the seeded mixture of tools/bench_ivf.py: ``--nlist`` planted unit centres, every row its centre plus Gaussian
noise of the same length, the queries drawn the same way.  The lists are those of ``gallery.ivf(nlist)`` over the fp32 rows
(``Int8IVFIndex.from_gallery``); the fp16 index is given the same centroids and assignments.

Per rows: one line with the sizes, then for Q in {1, 256} and nprobe in {1, 8, 32} at k = 3 one JSON line with

  i8_ms / i8_scan_ms ....... ``Int8IVFIndex.search(q, k, nprobe)`` / ``mi355_ivf_scan_i8`` alone, the probes given
  f16_ms / f16_scan_ms ..... ``IVFIndex.search`` over the fp16 gallery / its scan alone: the format a user would otherwise pick
  f32_ms / f32_scan_ms ..... the same over the fp32 gallery
  i8_exhaustive_ms ......... ``Int8Gallery.search(q, k)``
  i8_refined_ms ............ ``Int8IVFIndex.search(q, k, nprobe, refine=fp32 gallery)`` (to set beside f32_ms)
  recall_* ................. recall@k against the fp32 exhaustive search: of the int8 index raw and refined, of the fp16 and
                             fp32 indexes, and of the exhaustive int8 search
  rows_read ................ gallery rows the int8 scan streams (every list once per group of up to 8 of its queries)
  i8_gbps / f16_gbps / f32_gbps .. bytes of rows a scan streams (its own group size: 8, 4, 4) / its scan time
  i8_vs_f16 ................ f16_ms / i8_ms: above 1 the int8 index is the faster search

The variants run in alternation, each repetition timed with HIP events after a warm-up round; medians are reported.

    python tools/bench_ivf_i8.py [--rows 100000 1000000] [--dim 1536] [--nlist 1024] [--reps 7] [--out profiles/ivf_i8_bench.txt]
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


def _rows_read(index, probes, group):
    """Rows one scan streams: every list once per group of up to ``group`` of the queries that probe it."""
    pairs = torch.bincount(probes.reshape(-1), minlength=index.nlist)
    return int((((pairs + group - 1) // group) * index.counts).sum())


def _recall(got, want):
    return round(float((got.unsqueeze(2) == want.unsqueeze(1)).any(1).double().mean()), 4)


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
        sys.exit("bench_ivf_i8.py measures on the GPU; there is none here")
    D, K, k = a.dim, a.nlist, a.k
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        lines.append(line)
        print(line, flush=True)

    centres = M.l2_normalize_rows(M.synth_fill(K * D, 5, synth.NORMAL, DEV).view(K, D))
    queries = _mixture(256, centres, 9)
    for n in a.rows:
        g32 = M.Gallery(D, DEV, capacity=n)
        g16 = M.Gallery(D, DEV, capacity=n, dtype=torch.float16)
        for r0 in range(0, n, PIECE):
            x = _mixture(min(PIECE, n - r0), centres, 100 + r0 // PIECE, first=r0)
            g32.add(x)
            g16.add(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix8 = M.Int8IVFIndex.from_gallery(g32, K, iters=a.iters, seed=0)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        ix32 = g32.ivf(K, iters=a.iters, seed=0)                       # the cached index from_gallery took its lists from
        ix16 = M.IVFIndex(g16, ix32.centroids, ix32.assignments)
        i8 = ix8.i8
        counts = ix8.counts.cpu()
        emit({"rows": n, "D": D, "nlist": K, "kmeans_iters": a.iters, "build_s": round(build_s, 3), "index_bytes": ix8.nbytes,
              "i8_gallery_bytes": i8.nbytes, "f16_gallery_bytes": g16.nbytes, "f32_gallery_bytes": g32.nbytes,
              "list_rows_min": int(counts.min()), "list_rows_median": int(counts.median()), "list_rows_max": int(counts.max())})
        for Q in (1, 256):
            q = queries[:Q].contiguous()
            exact = g32.search(q, k)[1]
            for nprobe in (1, 8, 32):
                probes = ix8.probe(q, nprobe)
                cap = max(int(ix8._longest[nprobe]), k)
                runs = {
                    "i8": lambda: ix8.search(q, k, nprobe),
                    "i8_scan": lambda: ix8._scan(q, probes, cap, 0, None),
                    "f16": lambda: ix16.search(q, k, nprobe),
                    "f16_scan": lambda: ix16._scan(q, probes, cap, 0, None),
                    "f32": lambda: ix32.search(q, k, nprobe),
                    "f32_scan": lambda: ix32._scan(q, probes, cap, 0, None),
                    "i8_exhaustive": lambda: i8.search(q, k),
                    "i8_refined": lambda: ix8.search(q, k, nprobe, refine=g32),
                }
                t = {key: [] for key in runs}
                out = {}
                for rep in range(a.reps + 1):                          # the first round is the warm-up
                    for key, fn in runs.items():
                        ms, out[key] = _timed(fn)
                        if rep:
                            t[key].append(ms)
                rec = {"rows": n, "D": D, "nlist": K, "Q": Q, "nprobe": nprobe, "k": k, "reps": a.reps, "cap": cap}
                rec.update({f"{key}_ms": round(statistics.median(v), 4) for key, v in t.items()})
                rec["i8_vs_f16"] = round(rec["f16_ms"] / rec["i8_ms"], 2)
                rec["i8_scan_vs_f16_scan"] = round(rec["f16_scan_ms"] / rec["i8_scan_ms"], 2)
                rec["i8_refined_vs_f32"] = round(rec["f32_ms"] / rec["i8_refined_ms"], 2)
                for name, key in (("i8", "i8"), ("i8_refined", "i8_refined"), ("f16", "f16"), ("f32", "f32"),
                                  ("i8_exhaustive", "i8_exhaustive")):
                    rec[f"recall_{name}"] = _recall(out[key][1], exact)
                rec["rows_read"] = _rows_read(ix8, probes, 8)
                rec["gallery_rows"] = n
                rec["i8_gbps"] = round(rec["rows_read"] * i8._ld / rec["i8_scan_ms"] * 1e-6, 1)
                rec["f16_gbps"] = round(_rows_read(ix16, probes, 4) * g16._ld * 2 / rec["f16_scan_ms"] * 1e-6, 1)
                rec["f32_gbps"] = round(_rows_read(ix32, probes, 4) * g32._ld * 4 / rec["f32_scan_ms"] * 1e-6, 1)
                emit(rec)
        del ix8, ix16, ix32, i8, g16, g32
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_ivf_i8.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
