"""Search time, resident bytes and recall of the fp4 resident gallery (developer tool): ``FP4Gallery`` beside ``Int8Gallery``, the
fp16 ``Gallery`` and the asymmetric search of a ``BinaryGallery`` on the same synthetic rows and queries.  The variants run in
alternation in one process, each rep timed with HIP events around ``--calls`` back-to-back searches; the median of the reps is
reported, one JSON line per cell: the plain top-k, and the top-k of a shortlist rescored against the fp16 rows (``refine=``),
with recall@k of each against the fp32 gallery's search and the ratios against int8 (above 1: fp4 is the faster one).

    python tools/bench_rank_fp4.py [--rows clusters] [--cases 256x100000,256x1000000,1x1000000] [--k 3] [--shortlist 100]
                                   [--reps 9] [--calls 5] [--out profiles/rank_fp4_bench.txt]

``normal``: N(0,1) rows and queries.  ``clusters``: 1000 N(0,1) centres, each row and query a centre plus N(0,1).
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


def _rows(n, seed, kind, dev):
    x = M.synth_fill(n * D, seed, synth.NORMAL, dev).view(n, D)
    if kind == "clusters":
        centres = M.synth_fill(CENTRES * D, 3, synth.NORMAL, dev).view(CENTRES, D)
        pick = torch.randint(0, CENTRES, (n,), generator=torch.Generator().manual_seed(seed)).to(dev)
        for a in range(0, n, 1 << 16):                   # in blocks: no second (n, D) temporary
            x[a: a + (1 << 16)] += centres[pick[a: a + (1 << 16)]]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="clusters")
    ap.add_argument("--cases", default="256x100000,256x1000000,1x1000000")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--shortlist", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    sink = open(a.out, "w") if a.out else None
    k, R = a.k, a.shortlist

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    cases = [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")]
    for kind in a.rows.split(","):
        for G in sorted({g for _, g in cases}):
            x = _rows(G, 5, kind, dev)
            g32 = M.Gallery(D, dev, capacity=G).add(x)
            g16 = M.Gallery(D, dev, capacity=G, dtype=torch.float16).add(x)
            g8 = M.Int8Gallery(D, dev, capacity=G).add(x)
            g4 = M.FP4Gallery(D, dev, capacity=G).add(x)
            bg = M.BinaryGallery(D, dev, capacity=G)
            bg.train(x)
            bg.add(x)
            del x
            emit({"rows": kind, "G": G, "D": D,
                  "bytes_per_row": {"fp32": 4 * D, "fp16": g16.nbytes // G, "int8": g8.nbytes // G, "fp4": g4.nbytes // G,
                                    "binary": 4 * M.binary.row_words(D)}})
            for Q in [q for q, g in cases if g == G]:
                q = _rows(Q, 13, kind, dev)
                variants = {"fp16": lambda: g16.search(q, k)}
                for name, g in (("fp4", g4), ("int8", g8)):
                    variants[name] = lambda g=g: g.search(q, k)
                    variants[f"{name}_refined"] = lambda g=g: g.search(q, k, refine=g16, shortlist=R)
                variants["binary_asym"] = lambda: bg.search(q, k, asymmetric=True)
                variants["binary_asym_refined"] = lambda: bg.search(q, k, refine=g16, shortlist=R, asymmetric=True)
                for fn in variants.values():             # warm-up (the first calls of a process run slower)
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
                out = {"rows": kind, "Q": Q, "G": G, "D": D, "k": k, "shortlist": R, "reps": a.reps, "calls": a.calls}
                med = {name: statistics.median(v) for name, v in times.items()}
                for name, ms in med.items():
                    out[f"{name}_ms"] = round(ms, 4)
                want = g32.search(q, k)[1]
                for name, fn in variants.items():
                    out[f"{name}_recall_at_{k}"] = round(M.rank._recall(fn()[1], want, k)[0], 4)
                out["fp4_gallery_GBps"] = round(1.0 * G * (D // 2) / med["fp4"] / 1e6, 1)
                for other in ("int8", "fp16", "binary_asym"):
                    out[f"fp4_vs_{other}"] = round(med[other] / med["fp4"], 3)
                for other in ("int8", "binary_asym"):
                    out[f"fp4_refined_vs_{other}_refined"] = round(med[f"{other}_refined"] / med["fp4_refined"], 3)
                emit(out)
                del variants
            del g32, g16, g8, g4, bg
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
