"""Search time, index size and recall of the IVF-PQ index (developer tool): ``IVFPQIndex.search`` against the exhaustive
``PQGallery.search`` over the same codes and against ``Int8Gallery.search``, on the same synthetic rows and queries.  The
variants run in alternation in one process, each rep timed with HIP events around ``--calls`` back-to-back searches, after a
warm-up of every variant; the median of the reps is reported, one JSON line per (Q, k), with recall@k of every IVF-PQ variant
against the fp32 gallery's search and against the exhaustive PQ search, and one line per index with its build time (the k-means
of the fp32 gallery, then the lists and the list-ordered copy of the codes) and its bytes.

    python tools/bench_ivfpq.py [--rows clusters] [--G 100000,1000000] [--Q 1,16,256] [--k 3,150] [--M 48,96]
                                [--nlist 256,1024] [--nprobe 1,8,32] [--train-rows 100000] [--pq-iters 10] [--iters 10]
                                [--reps 9] [--calls 5] [--only ivfpq] [--out profiles/ivfpq_bench.txt]

``IVFPQIndex.search`` reads one flag word back at the end of every call, so its back-to-back calls do not overlap on the host
as those of the other two do: the time of a call includes that round trip.  Rows as in tools/bench_pq.py.  ``--only ivfpq``
times the IVF-PQ variants alone and skips the recall (for a kernel trace that holds no other search's launches).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from bench_pq import D, _ints, _rows, _timed  # noqa: E402


def _recall(got, want):
    k = want.shape[1]
    return float(((got.unsqueeze(2) == want.unsqueeze(1)).any(dim=1).sum(dim=1).double() / float(k)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="clusters")
    ap.add_argument("--G", default="100000,1000000")
    ap.add_argument("--Q", default="1,16,256")
    ap.add_argument("--k", default="3,150")
    ap.add_argument("--M", default="48,96")
    ap.add_argument("--nlist", default="256,1024")
    ap.add_argument("--nprobe", default="1,8,32")
    ap.add_argument("--train-rows", type=int, default=100000)
    ap.add_argument("--pq-iters", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default=None, help="time only the variants whose name starts with this; no recall")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    sink = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for kind in a.rows.split(","):
        for G in _ints(a.G):
            x = _rows(G, 5, kind, dev)
            g32 = M.Gallery(D, dev, capacity=G).add(x)
            g8 = M.Int8Gallery(D, dev, capacity=G).add(x)
            pqs = {}
            for m in _ints(a.M):
                pqs[m] = M.PQGallery(D, dev, m, capacity=G).train(x[:min(G, a.train_rows)], iters=a.pq_iters).add(x)
            del x
            g32.kmeans(8, iters=1)                                   # warm-up of the clustering kernels
            torch.cuda.synchronize()
            idx = {}
            for nlist in _ints(a.nlist):
                km, kmeans_ms = _timed(lambda: g32.kmeans(nlist, iters=a.iters))
                for m, g in pqs.items():
                    ix, lists_ms = _timed(lambda: M.IVFPQIndex(g, km.centroids, km.assignments))
                    idx[(m, nlist)] = ix
                    counts = ix.counts
                    emit({"rows": kind, "G": G, "D": D, "M": m, "nlist": nlist, "iters": a.iters, "kmeans_ms": round(kmeans_ms, 1),
                          "lists_ms": round(lists_ms, 1), "build_ms": round(kmeans_ms + lists_ms, 1), "index_nbytes": ix.nbytes,
                          "list_codes_nbytes": ix.list_codes.numel(), "pq_nbytes": g.nbytes, "int8_nbytes": g8.nbytes,
                          "longest_list": int(counts.max()), "empty_lists": int((counts == 0).sum())})
            for Q in _ints(a.Q):
                q = _rows(Q, 13, kind, dev)
                for k in _ints(a.k):
                    variants = {"int8": lambda: g8.search(q, k)}
                    for m, g in pqs.items():
                        variants[f"pq{m}"] = lambda g=g: g.search(q, k)
                    for (m, nlist), ix in idx.items():
                        for nprobe in _ints(a.nprobe):
                            variants[f"ivfpq{m}_l{nlist}_p{nprobe}"] = lambda ix=ix, nprobe=nprobe: ix.search(q, k, nprobe)
                    if a.only:
                        variants = {name: fn for name, fn in variants.items() if name.startswith(a.only)}
                    for fn in variants.values():         # warm-up (the first calls of a process run slower)
                        for _ in range(3):
                            fn()
                    torch.cuda.synchronize()
                    times = {name: [] for name in variants}
                    for _ in range(a.reps):
                        for name, fn in variants.items():
                            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            t0.record()
                            for _ in range(a.calls):
                                fn()
                            t1.record()
                            t1.synchronize()
                            times[name].append(t0.elapsed_time(t1) / a.calls)
                    med = {name: statistics.median(v) for name, v in times.items()}
                    out = {"rows": kind, "Q": Q, "G": G, "D": D, "k": k, "reps": a.reps, "calls": a.calls}
                    if a.only:
                        out.update({f"{name}_ms": round(ms, 4) for name, ms in med.items()})
                        emit(out)
                        continue
                    for name in ("int8",) + tuple(f"pq{m}" for m in pqs):
                        out[f"{name}_ms"] = round(med[name], 4)
                    exact = g32.search(q, k)[1]
                    for m, g in pqs.items():
                        whole = g.search(q, k)[1]
                        out[f"pq{m}_recall_at_{k}"] = round(_recall(whole, exact), 4)
                        for (mm, nlist), ix in idx.items():
                            if mm != m:
                                continue
                            for nprobe in _ints(a.nprobe):
                                name = f"ivfpq{m}_l{nlist}_p{nprobe}"
                                got = ix.search(q, k, nprobe)[1]
                                out[name] = {"ms": round(med[name], 4), "vs_pq": round(med[f"pq{m}"] / med[name], 3),
                                             "vs_int8": round(med["int8"] / med[name], 3),
                                             f"recall_at_{k}_vs_fp32": round(_recall(got, exact), 4),
                                             f"recall_at_{k}_vs_pq": round(_recall(got, whole), 4)}
                    emit(out)
            del g32, g8, pqs, idx, variants
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
