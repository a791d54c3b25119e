"""Search time and recall of the int8 resident gallery (developer tool): fp32 ``Gallery``, fp16 ``Gallery`` and ``Int8Gallery``
on the same synthetic rows and queries.  The variants run in alternation in one process, each rep timed with HIP events around
``--calls`` back-to-back searches; the median of the reps is reported, one JSON line per case, with recall@k of the int8
search against the fp32 gallery's search.

    python tools/bench_rank_i8.py [--rows normal|clusters] [--reps 15] [--calls 10]
                                  [--cases 256x100000x3,1x100000x3,256x100000x150,256x1000000x3]

``--rows normal``: N(0,1) rows and queries.  ``--rows clusters``: 1000 N(0,1) centres, each row and query a centre plus N(0,1).
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
    ap.add_argument("--rows", choices=("normal", "clusters"), default="normal")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cases", default="256x100000x3,1x100000x3,256x100000x150,256x1000000x3")
    a = ap.parse_args()
    dev = "cuda:0"
    for case in a.cases.split(","):
        Q, G, k = (int(v) for v in case.split("x"))
        q = _rows(Q, 13, a.rows, dev)
        x = _rows(G, 5, a.rows, dev)
        g32 = M.Gallery(D, dev, capacity=G).add(x)
        g16 = M.Gallery(D, dev, capacity=G, dtype=torch.float16).add(x)
        g8 = M.Int8Gallery(D, dev, capacity=G).add(x)
        del x
        variants = {"fp32": lambda: g32.search(q, k), "fp16": lambda: g16.search(q, k), "int8": lambda: g8.search(q, k)}
        for fn in variants.values():                     # warm-up (the first calls of a process run slower)
            for _ in range(10):
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
        out = {"rows": a.rows, "Q": Q, "G": G, "D": D, "k": k, "reps": a.reps, "calls": a.calls}
        for name, ms in med.items():
            out[f"{name}_ms"] = round(ms, 4)
            out[f"{name}_qps"] = round(Q / ms * 1e3, 1)
        out["int8_speedup_vs_fp32"] = round(med["fp32"] / med["int8"], 3)
        out["int8_speedup_vs_fp16"] = round(med["fp16"] / med["int8"], 3)
        out["int8_gallery_GBps"] = round(1.0 * G * D / med["int8"] / 1e6, 1)
        out[f"int8_recall_at_{k}"] = round(g8.recall(q, k, g32)[0], 4)
        out["nbytes"] = {"fp32": g32.nbytes, "fp16": g16.nbytes, "int8": g8.nbytes}
        print(json.dumps(out), flush=True)
        del g32, g16, g8, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
