"""Verification ROC timings (developer tool): ``verification_roc`` (the histogram inside the cosine GEMM's epilogue) at
T = 21 and T = 4096 next to ``cosine_topk`` k = 3 (the fused top-k epilogue it stands beside) and next to materialising
``cosine_scores`` and counting with torch (searchsorted + bincount), all on the same rows.  The variants run in
alternation, each rep timed with HIP events around ``--calls`` back-to-back calls; the median of the reps is reported, one
JSON line per case.  Then the same-source ``--square`` call (rows x rows) and ``roc_curve`` on ``--pairs`` given scores.

    python tools/bench_verification.py [--reps 15] [--calls 5] [--cases 256x100000] [--square 100000] [--pairs 100000000]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import synth  # noqa: E402

D = 1536
T4096 = np.linspace(-0.2, 0.2, 4096)


def _time(variants, reps, calls):
    for fn in variants.values():                         # warm-up (the first calls of a process run slower)
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


def _slab_count(q, g, ql, gl, thr):
    S = M.cosine_scores(q, g)
    b = torch.searchsorted(thr, S.double(), right=True)
    gen = ql[:, None] == gl[None, :]
    n = thr.numel() + 1
    return torch.bincount(b[gen], minlength=n), torch.bincount(b[~gen], minlength=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", default="256x100000")
    ap.add_argument("--square", type=int, default=100000)
    ap.add_argument("--pairs", type=int, default=100000000)
    a = ap.parse_args()
    dev = "cuda:0"
    for case in a.cases.split(","):
        Q, G = (int(v) for v in case.split("x"))
        q = M.synth_fill(Q * D, 13, synth.NORMAL, dev).view(Q, D)
        g = M.synth_fill(G * D, 5, synth.NORMAL, dev).view(G, D)
        ql = torch.arange(Q, device=dev) % 1000
        gl = torch.arange(G, device=dev) % 1000
        t21 = torch.as_tensor(np.array(list(range(0, 105, 5))) / 100, device=dev)
        variants = {
            "roc_t21": lambda: M.verification_roc(q, ql, g, gl),
            "roc_t4096": lambda: M.verification_roc(q, ql, g, gl, thresholds=T4096),
            "topk_k3": lambda: M.cosine_topk(q, g, 3),
            "slab_torch_t21": lambda: _slab_count(q, g, ql, gl, t21),
        }
        med = _time(variants, a.reps, a.calls)
        out = {"Q": Q, "G": G, "D": D, "reps": a.reps, "calls": a.calls}
        out.update({f"{k}_ms": round(v, 4) for k, v in med.items()})
        out["roc_t21_over_topk"] = round(med["roc_t21"] / med["topk_k3"], 3)
        out["roc_t4096_over_topk"] = round(med["roc_t4096"] / med["topk_k3"], 3)
        print(json.dumps(out), flush=True)
        del q, g
        torch.cuda.empty_cache()
    if a.square:
        n = a.square
        x = M.synth_fill(n * D, 7, synth.NORMAL, dev).view(n, D)
        lab = torch.arange(n, device=dev) % 1000
        med = _time({"t21": lambda: M.verification_roc(x, lab), "t4096": lambda: M.verification_roc(x, lab, thresholds=T4096)},
                    3, 1)
        print(json.dumps({"same_source": f"{n}x{n}x{D}", "pairs": n * (n - 1), **{f"{k}_ms": round(v, 2) for k, v in med.items()}}),
              flush=True)
        del x
        torch.cuda.empty_cache()
    if a.pairs:
        n = a.pairs
        s = (M.synth_fill(n, 3, synth.UNIFORM, dev) * 2 - 1).contiguous()
        act = (M.synth_fill(n, 4, synth.UNIFORM, dev) < 0.5).to(torch.int8)
        s64 = s.double()
        med = _time({"fp32_t21": lambda: M.roc_curve(s, act), "fp32_t4096": lambda: M.roc_curve(s, act, thresholds=T4096),
                     "fp64_t21": lambda: M.roc_curve(s64, act)}, a.reps, 1)
        print(json.dumps({"roc_curve_pairs": n, **{f"{k}_ms": round(v, 3) for k, v in med.items()}}), flush=True)


if __name__ == "__main__":
    main()
