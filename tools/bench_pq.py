"""Search time, resident bytes and recall of the product-quantised gallery (developer tool): fp32 ``Gallery``, fp16 ``Gallery``,
``Int8Gallery`` and ``PQGallery`` (M = 48 and 96) on the same synthetic rows and queries.  The variants run in alternation in
one process, each rep timed with HIP events around ``--calls`` back-to-back searches; the median of the reps is reported, one
JSON line per case, with recall@k of the raw PQ search and of the refined one (shortlist 100, rescored against the fp16 rows)
against the fp32 gallery's search, and one line per gallery with the training and encoding times.

    python tools/bench_pq.py [--rows normal,clusters] [--G 100000,1000000] [--Q 1,16,256] [--k 3,150] [--M 48,96]
                             [--train-rows 100000] [--iters 10] [--reps 9] [--calls 5] [--out profiles/pq_bench.txt]

``normal``: N(0,1) rows and queries.  ``clusters``: 1000 N(0,1) centres, each row and query a centre plus N(0,1).  The
codebooks are trained on the first ``--train-rows`` rows of the gallery.
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

D = 1536
CENTRES = 1000
SHORTLIST = 100


def _rows(n, seed, kind, dev):
    x = M.synth_fill(n * D, seed, synth.NORMAL, dev).view(n, D)
    if kind == "clusters":
        centres = M.synth_fill(CENTRES * D, 3, synth.NORMAL, dev).view(CENTRES, D)
        pick = torch.randint(0, CENTRES, (n,), generator=torch.Generator().manual_seed(seed)).to(dev)
        for a in range(0, n, 1 << 16):                   # in blocks: no second (n, D) temporary
            x[a: a + (1 << 16)] += centres[pick[a: a + (1 << 16)]]
    return x


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    r = fn()
    t1.record()
    t1.synchronize()
    return r, t0.elapsed_time(t1)


def _ints(s):
    return [int(v) for v in s.split(",")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="normal,clusters")
    ap.add_argument("--G", default="100000,1000000")
    ap.add_argument("--Q", default="1,16,256")
    ap.add_argument("--k", default="3,150")
    ap.add_argument("--M", default="48,96")
    ap.add_argument("--train-rows", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
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
            g16 = M.Gallery(D, dev, capacity=G, dtype=torch.float16).add(x)
            g8 = M.Int8Gallery(D, dev, capacity=G).add(x)
            pqs = {}
            for m in _ints(a.M):
                g = M.PQGallery(D, dev, m, capacity=G)
                n_train = min(G, a.train_rows)
                g.train(x[:256], iters=1)                 # warm-up of the training kernels
                torch.cuda.synchronize()
                _, train_ms = _timed(lambda: g.train(x[:n_train], iters=a.iters))
                _, encode_ms = _timed(lambda: g.add(x))
                pqs[m] = g
                emit({"rows": kind, "G": G, "D": D, "M": m, "train_rows": n_train, "iters": a.iters, "train_ms": round(train_ms, 1),
                      "encode_ms": round(encode_ms, 1), "nbytes": {"fp32": g32.nbytes, "fp16": g16.nbytes, "int8": g8.nbytes,
                                                                     f"pq{m}": g.nbytes}})
            del x
            for Q in _ints(a.Q):
                q = _rows(Q, 13, kind, dev)
                for k in _ints(a.k):
                    variants = {"fp32": lambda: g32.search(q, k), "fp16": lambda: g16.search(q, k), "int8": lambda: g8.search(q, k)}
                    for m, g in pqs.items():
                        variants[f"pq{m}"] = lambda g=g: g.search(q, k)
                        variants[f"pq{m}_refined"] = lambda g=g: g.search(q, k, refine=g16, shortlist=max(SHORTLIST, k))
                    for fn in variants.values():         # warm-up (the first calls of a process run slower)
                        for _ in range(5):
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
                    out = {"rows": kind, "Q": Q, "G": G, "D": D, "k": k, "reps": a.reps, "calls": a.calls,
                           "shortlist": max(SHORTLIST, k)}
                    med = {name: statistics.median(v) for name, v in times.items()}
                    for name, ms in med.items():
                        out[f"{name}_ms"] = round(ms, 4)
                    for m, g in pqs.items():
                        out[f"pq{m}_vs_int8"] = round(med["int8"] / med[f"pq{m}"], 3)
                        out[f"pq{m}_recall_at_{k}"] = round(g.recall(q, k, g32)[0], 4)
                        out[f"pq{m}_refined_recall_at_{k}"] = round(g.recall(q, k, g32, refine=g16, shortlist=max(SHORTLIST, k))[0], 4)
                    emit(out)
            del g32, g16, g8, pqs, variants
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
