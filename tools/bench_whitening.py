"""PCA whitening timings (developer tool).  One JSON line per case:

* ``moments``: ``embedding_moments`` at R rows, D in {1536, 2560}, fp32 rows and fp16 gallery rows, next to the same arithmetic
  through torch on the same card in the same process (``x.double().T @ x.double()``); the f64 FLOP rate counts the upper
  triangle the kernel computes (R * D * (D + 1)) and, for torch, the whole product (2 * R * D * D).
* ``transform``: ``Whitening.transform`` at (1536 -> 256) and (1536 -> 1536) next to ``normalize(normalize(x) @ W.T + b)`` in torch.
* ``search``: ``Gallery.search`` of 256 queries, k = 3, against R x 1536 and R x 256 rows (the existing kernels: what the
  reduction buys), fp32 and fp16 galleries.

Variants run in alternation, each rep timed with HIP events; the median of the reps is reported (after warm-up).

    python tools/bench_whitening.py [--reps 20] [--rows 100000] [--out profiles/FILE]
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


def _time(variants, reps, calls=1):
    for fn in variants.values():
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


def _random_whitening(D, d, dev):
    w = M.Whitening()
    w.dim_in, w.dim_out, w.num_rows = D, d, 2
    w.matrix = M.synth_fill(d * D, 7, synth.NORMAL, dev).view(d, D).contiguous()
    w.bias = M.synth_fill(d, 8, synth.NORMAL, dev)
    w.mean = torch.zeros(D, device=dev)
    w.eigenvalues = torch.ones(D, dtype=torch.float64)
    w.explained_variance_ratio = torch.ones(d, dtype=torch.float64) / D
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    R = a.rows
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    for D in (1536, 2560):
        x = M.synth_fill(R * D, 1, synth.NORMAL, dev).view(R, D)
        g16 = M.Gallery(D, dev, capacity=R, dtype=torch.float16).add(x)
        out = M.embedding_moments(x)
        t = _time({"fp32": lambda: M.embedding_moments(x, out=out), "fp32_normalize": lambda: M.embedding_moments(x, normalize=True, out=out),
                   "fp16": lambda: M.embedding_moments(g16, out=out),
                   "torch_f64": lambda: x.double().T @ x.double()}, a.reps)
        tri, full = R * D * (D + 1), 2.0 * R * D * D
        for name in ("fp32", "fp32_normalize", "fp16"):
            emit({"case": "moments", "rows": name, "R": R, "D": D, "ms": round(t[name], 3), "f64_TFLOPs": round(tri / t[name] / 1e9, 2),
                  "torch_ms": round(t["torch_f64"], 3), "torch_f64_TFLOPs": round(full / t["torch_f64"] / 1e9, 2),
                  "ratio_to_torch": round(t[name] / t["torch_f64"], 3)})
        del g16, out
        if D == 1536:
            for d in (256, 1536):
                w = _random_whitening(D, d, dev)
                y = torch.empty((R, d), device=dev)
                Wt, b = w.matrix.t().contiguous(), w.bias

                def via_torch():
                    return torch.nn.functional.normalize(torch.nn.functional.normalize(x, dim=1, eps=1e-6) @ Wt + b, dim=1, eps=1e-6)

                t = _time({"hip": lambda: w.transform(x, out=y), "torch": via_torch}, a.reps)
                flop = 2.0 * R * D * d
                emit({"case": "transform", "R": R, "D": D, "d": d, "ms": round(t["hip"], 3), "f32_TFLOPs": round(flop / t["hip"] / 1e9, 2),
                      "torch_ms": round(t["torch"], 3), "torch_TFLOPs": round(flop / t["torch"] / 1e9, 2),
                      "ratio_to_torch": round(t["hip"] / t["torch"], 3)})
                del y
            q = M.synth_fill(256 * D, 2, synth.NORMAL, dev).view(256, D)
            w = _random_whitening(D, 256, dev)
            for dt, name in ((torch.float32, "fp32"), (torch.float16, "fp16")):
                big = M.Gallery(D, dev, capacity=R, dtype=dt).add(x)
                small = big.whitened(w)
                tq = w.transform(q)
                t = _time({"big": lambda: big.search(q, 3), "small": lambda: small.search(tq, 3), "query_transform": lambda: w.transform(q)},
                          a.reps, calls=5)
                emit({"case": "search", "gallery": name, "Q": 256, "k": 3, "R": R, "ms_D1536": round(t["big"], 4),
                      "ms_D256": round(t["small"], 4), "query_transform_ms": round(t["query_transform"], 4),
                      "speedup": round(t["big"] / (t["small"] + t["query_transform"]), 2),
                      "MB_D1536": round(big.nbytes / 1e6, 1), "MB_D256": round(small.nbytes / 1e6, 1)})
                del big, small
        del x
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
