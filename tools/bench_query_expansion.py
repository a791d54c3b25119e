"""Alpha query expansion / DBA timings (developer tool).  Three cases, one JSON line each:

* ``kernel``: ``mi355_expand_rows`` alone on fixed neighbour lists, Q = 256, n in {1, 10, 64}, G = 100k, D = 1536, fp32 and
  fp16 galleries; bytes per query = n * D * elem gathered + D * 4 base + 4 * D * 4 (x stored, read by the norm, read and
  rewritten scaled); GB/s and the fraction of the 8 TB/s HBM peak.
* ``qe_search``: ``Gallery.search(q, k, qe=(n, alpha))`` end to end next to two plain searches (k = 3, n = 10).
* ``dba``: ``Gallery.augmented(n)`` at G = 100k, split into the self-join (the blocked ``exclude=arange`` searches) and the
  expansion launches.

Variants run in alternation, each rep timed with HIP events around ``--calls`` back-to-back calls; the median of the reps is
reported (after warm-up).

    python tools/bench_query_expansion.py [--reps 15] [--calls 5] [--rows 100000] [--out profiles/FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import rank as R  # noqa: E402
from imageretrievalresearch_amd import synth  # noqa: E402

D = 1536
PEAK = 8.0e12


def _time(variants, reps, calls):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    G, Q = a.rows, 256
    lines = []

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        lines.append(s)

    g = M.synth_fill(G * D, 1, synth.NORMAL, dev).view(G, D)
    q = M.synth_fill(Q * D, 2, synth.NORMAL, dev).view(Q, D)
    gals = {"fp32": M.Gallery(D, dev, capacity=G).add(g), "fp16": M.Gallery(D, dev, capacity=G, dtype=torch.float16).add(g)}
    del g
    gen = torch.Generator(device=dev).manual_seed(3)
    # 1. the kernel alone: random rows, positive scores (every slot used)
    for name, gal in gals.items():
        elem = 4 if gal.dtype == torch.float32 else 2
        for n in (1, 10, 64):
            idx = torch.randint(0, G, (Q, n), device=dev, generator=gen)
            vals = torch.rand((Q, n), device=dev, generator=gen) * 0.5 + 0.4
            out = torch.empty((Q, D), device=dev)
            t = _time({"k": lambda: R._expand_rows(q, True, gal._buf, gal.dtype, G, D, vals, idx, 3.0, gal.eps, out=out)},
                      a.reps, a.calls)["k"]
            nbytes = Q * (n * D * elem + D * 4 + 4 * D * 4)   # neighbours, base; store x, norm read, scale read + write
            gbs = nbytes / (t * 1e-3) / 1e9
            emit({"case": "kernel", "gallery": name, "Q": Q, "n": n, "G": G, "D": D, "ms": round(t, 4), "MB": round(nbytes / 1e6, 2),
                  "GBps": round(gbs, 1), "frac_peak": round(gbs * 1e9 / PEAK, 4)})
    # 2. QE search end to end against two plain searches
    for name, gal in gals.items():
        r = _time({"qe": lambda: gal.search(q, 3, qe=(10, 3.0)),
                   "two_plain": lambda: (gal.search(q, 10), gal.search(q, 3))}, a.reps, a.calls)
        emit({"case": "qe_search", "gallery": name, "Q": Q, "k": 3, "n": 10, "G": G, "D": D, "qe_ms": round(r["qe"], 4),
              "two_plain_ms": round(r["two_plain"], 4), "ratio": round(r["qe"] / r["two_plain"], 3)})
    # 3. DBA at G rows: the whole call, and its self-join alone (blocks of 256)
    for name, gal in gals.items():
        ex_all = torch.arange(G, dtype=torch.int64, device=dev)

        def self_join():
            for q0 in range(0, G, 256):
                rows = gal._buf[q0: q0 + 256]
                ex = ex_all[q0: q0 + rows.shape[0]]
                if gal.dtype == torch.float16:
                    gal.search(rows[:, :D].float(), 10, exclude=ex)
                else:
                    M.cosine_topk(rows, gal.data, 10, gal.eps, gallery_is_normalized=True, exclude=ex)

        r = _time({"dba": lambda: gal.augmented(10, 3.0), "self_join": self_join}, max(3, a.reps // 5), 1)
        emit({"case": "dba", "gallery": name, "G": G, "D": D, "n": 10, "total_ms": round(r["dba"], 2),
              "self_join_ms": round(r["self_join"], 2), "expansion_ms": round(r["dba"] - r["self_join"], 2)})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
