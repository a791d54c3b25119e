"""Cosine range search timings (developer tool): ``cosine_range`` (hits kept inside the cosine GEMM's epilogue, then the
compaction) at thresholds that give about 0, 10 and 1000 hits per query, next to materialising ``cosine_scores`` and taking
``torch.nonzero`` of ``S >= t`` (plus the scores) on the same rows, next to ``cosine_topk`` k = 3 (the fused top-k epilogue),
and the same shapes against an fp16 ``Gallery``.  The variants run in alternation, each rep timed with HIP events around
``--calls`` back-to-back calls; the median of the reps is reported, one JSON line per case.  Then a ``--square`` self-join
(rows x rows, ``exclude=arange``, ``label_filter="different"``).  ``--profile`` only runs range and top-k a few times (for
``rocprofv3 --kernel-trace --stats``).

    python tools/bench_range.py [--reps 15] [--calls 5] [--cases 256x100000] [--square 100000] [--profile]
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
HITS = (0, 10, 1000)                                     # hits per query the thresholds aim at


def _time(variants, reps, calls):
    for fn in variants.values():                         # warm-up (also grows the cached candidate buffer)
        for _ in range(3):
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
    return {name: statistics.median(v) for name, v in times.items()}


def _slab_nonzero(q, g, t):
    S = M.cosine_scores(q, g)
    qi, gi = (S >= t).nonzero(as_tuple=True)
    return qi, gi, S[qi, gi]


def _thresholds(q, g):
    """Thresholds with about h hits per query (h = 0: one above every score)."""
    S = M.cosine_scores(q, g).flatten()
    out = {}
    for h in HITS:
        out[h] = 0.5 if h == 0 else float(S.kthvalue(S.numel() - h * q.shape[0] + 1).values)
    del S
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", default="256x100000")
    ap.add_argument("--square", type=int, default=100000)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    for case in a.cases.split(","):
        Q, G = (int(v) for v in case.split("x"))
        q = M.synth_fill(Q * D, 13, synth.NORMAL, dev).view(Q, D)
        g = M.synth_fill(G * D, 5, synth.NORMAL, dev).view(G, D)
        if a.profile:
            t = _thresholds(q, g)[10]
            for _ in range(10):
                M.cosine_range(q, g, t)
                M.cosine_topk(q, g, 3)
            torch.cuda.synchronize()
            print(json.dumps({"profile": case, "t": t}), flush=True)
            return
        g16 = M.Gallery(D, dev, dtype=torch.float16).add(g)
        for h, t in _thresholds(q, g).items():
            variants = {
                "range": lambda: M.cosine_range(q, g, t),
                "slab_nonzero": lambda: _slab_nonzero(q, g, t),
                "topk_k3": lambda: M.cosine_topk(q, g, 3),
                "range_f16": lambda: g16.range_search(q, t),
                "topk_k3_f16": lambda: g16.search(q, 3),
            }
            med = _time(variants, a.reps, a.calls)
            nnz = int(M.cosine_range(q, g, t).offsets[-1])
            nnz16 = int(g16.range_search(q, t).offsets[-1])
            out = {"Q": Q, "G": G, "D": D, "hits_per_query_target": h, "threshold": round(t, 6), "nnz": nnz, "nnz_f16": nnz16,
                   "reps": a.reps, "calls": a.calls}
            out.update({f"{k}_ms": round(v, 4) for k, v in med.items()})
            out["range_over_topk"] = round(med["range"] / med["topk_k3"], 3)
            out["range_f16_over_topk_f16"] = round(med["range_f16"] / med["topk_k3_f16"], 3)
            out["slab_nonzero_over_range"] = round(med["slab_nonzero"] / med["range"], 2)
            print(json.dumps(out), flush=True)
        del q, g, g16
        torch.cuda.empty_cache()
    if a.square:
        n = a.square
        x = M.synth_fill(n * D, 7, synth.NORMAL, dev).view(n, D)
        lab = torch.arange(n, device=dev) % 1000
        ex = torch.arange(n, device=dev)
        t = 0.12
        run = lambda: M.cosine_range(x, x, t, query_labels=lab, gallery_labels=lab, label_filter="different",  # noqa: E731
                                     exclude=ex)
        med = _time({"self_join": run}, 3, 1)
        r = run()
        print(json.dumps({"self_join": f"{n}x{n}x{D}", "threshold": t, "nnz": int(r.offsets[-1]),
                          "ms": round(med["self_join"], 2)}), flush=True)


if __name__ == "__main__":
    main()
