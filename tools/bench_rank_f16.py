"""Search time of the three resident-gallery formats (developer tool): fp32 ``Gallery``, ``PreparedGallery`` (bf16 planes)
and the fp16 ``Gallery``, on the same synthetic rows and queries.  The variants run in alternation, each rep timed with
HIP events around ``--calls`` back-to-back searches; the median of the reps is reported, one JSON line per case.

    python tools/bench_rank_f16.py [--reps 15] [--calls 10] [--cases 256x100000x3,1x100000x3,256x100000x150,256x1000000x3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cases", default="256x100000x3,1x100000x3,256x100000x150,256x1000000x3")
    a = ap.parse_args()
    dev = "cuda:0"
    for case in a.cases.split(","):
        Q, G, k = (int(v) for v in case.split("x"))
        q = M.synth_fill(Q * D, 13, synth.NORMAL, dev).view(Q, D)
        x = M.synth_fill(G * D, 5, synth.NORMAL, dev).view(G, D)
        g32 = M.Gallery(D, dev, capacity=G).add(x)
        g16 = M.Gallery(D, dev, capacity=G, dtype=torch.float16).add(x)
        del x
        variants = {"fp32": lambda: g32.search(q, k), "fp16": lambda: g16.search(q, k)}
        prepared = None
        if M.PreparedGallery.supports(Q, k):
            prepared = M.PreparedGallery(g32.data)
            variants["prepared"] = lambda: prepared.search(q, k)
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
        out = {"Q": Q, "G": G, "D": D, "k": k, "reps": a.reps, "calls": a.calls}
        for name, ms in med.items():
            out[f"{name}_ms"] = round(ms, 4)
            out[f"{name}_qps"] = round(Q / ms * 1e3, 1)
        out["fp16_speedup_vs_fp32"] = round(med["fp32"] / med["fp16"], 3)
        out["fp16_gallery_GBps"] = round(2.0 * G * D / med["fp16"] / 1e6, 1)
        out["nbytes"] = {"fp32": g32.nbytes, "fp16": g16.nbytes,
                         "prepared": prepared.planes.numel() if prepared is not None else None}
        print(json.dumps(out), flush=True)
        del g32, g16, prepared, variants
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
