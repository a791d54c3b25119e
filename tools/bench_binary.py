"""Search time, resident bytes and recall of the binary (sign-bit) gallery (developer tool): ``BinaryGallery`` beside the
galleries it has to be weighed against - fp16 ``Gallery``, ``Int8Gallery`` and ``PQGallery`` (M = 96) - on the same synthetic
rows and queries, in the same run.  The variants run in alternation in one process, each rep timed with HIP events around
``--calls`` back-to-back searches; the median of the reps is reported, one JSON line per cell: the plain searches at k, the
shortlist alone (the first stage of a refined search: k = ``--shortlist``), every ``refine=`` variant at that shortlist
(rescored against the fp16 rows), and recall@k of each against the fp32 gallery's search.  The asymmetric search of the same
binary codes (``asymmetric=True``: int8 query codes against the bits) runs in the same alternation - plain, shortlist, refined,
recall plain and refined - with its ratios against the symmetric search and against int8 (``binary_asym_*``; above 1: the
asymmetric search is the faster one).

    python tools/bench_binary.py [--rows clusters] [--G 100000,1000000] [--Q 1,256] [--k 3] [--shortlist 100] [--M 96]
                                 [--train-rows 100000] [--iters 10] [--reps 9] [--calls 5] [--out profiles/binary_bench.txt]

``normal``: N(0,1) rows and queries.  ``clusters``: 1000 N(0,1) centres, each row and query a centre plus N(0,1).  The
binary centre is trained on the whole gallery, the PQ codebooks on its first ``--train-rows`` rows.

What to expect, by counting instructions: a (query, row) pair at D = 1536 is 48 words x (xor + accumulating popcount), so 256
queries x 1M rows are 2.5e10 lane-operations against 256 CUs x 4 SIMDs x 32 lanes per clock: 0.3 - 0.6 ms at the clocks the
chip holds.  One query reads the codes once: 192 MB, tens of microseconds at HBM rate.
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
    ap.add_argument("--rows", default="clusters")
    ap.add_argument("--G", default="100000,1000000")
    ap.add_argument("--Q", default="1,256")
    ap.add_argument("--k", default="3")
    ap.add_argument("--shortlist", type=int, default=100)
    ap.add_argument("--M", type=int, default=96)
    ap.add_argument("--train-rows", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    sink = open(a.out, "w") if a.out else None
    R = a.shortlist

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
            pq = M.PQGallery(D, dev, a.M, capacity=G)
            n_train = min(G, a.train_rows)
            pq.train(x[:n_train], iters=a.iters)
            pq.add(x)
            bg = M.BinaryGallery(D, dev, capacity=G)
            bg.train(x[:256])                            # warm-up of the moments kernel
            torch.cuda.synchronize()
            _, train_ms = _timed(lambda: bg.train(x))
            bg.add(x[:256])                              # warm-up of the encoder (a throw-away gallery)
            bg = M.BinaryGallery(D, dev, center=bg.center, capacity=G)
            torch.cuda.synchronize()
            _, encode_ms = _timed(lambda: bg.add(x))
            emit({"rows": kind, "G": G, "D": D, "binary_train_ms": round(train_ms, 2), "binary_encode_ms": round(encode_ms, 2),
                  "bytes_per_row": {"fp32": 4 * D, "fp16": g16.nbytes // G, "int8": g8.nbytes // G, f"pq{a.M}": a.M,
                                    "binary": 4 * M.binary.row_words(D)},
                  "nbytes": {"fp32": g32.nbytes, "fp16": g16.nbytes, "int8": g8.nbytes, f"pq{a.M}": pq.nbytes, "binary": bg.nbytes}})
            del x
            for Q in _ints(a.Q):
                q = _rows(Q, 13, kind, dev)
                for k in _ints(a.k):
                    first = {"binary": bg, "int8": g8, f"pq{a.M}": pq}
                    variants = {"fp16": lambda: g16.search(q, k)}
                    for name, g in first.items():
                        variants[name] = lambda g=g: g.search(q, k)
                        variants[f"{name}_shortlist"] = lambda g=g: g.search(q, R)
                        variants[f"{name}_refined"] = lambda g=g: g.search(q, k, refine=g16, shortlist=R)
                    # the asymmetric search over the same codes: int8 query codes against the bits on the i8 MFMA
                    variants["binary_asym"] = lambda: bg.search(q, k, asymmetric=True)
                    variants["binary_asym_shortlist"] = lambda: bg.search(q, R, asymmetric=True)
                    variants["binary_asym_refined"] = lambda: bg.search(q, k, refine=g16, shortlist=R, asymmetric=True)
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
                    out = {"rows": kind, "Q": Q, "G": G, "D": D, "k": k, "shortlist": R, "reps": a.reps, "calls": a.calls}
                    med = {name: statistics.median(v) for name, v in times.items()}
                    for name, ms in med.items():
                        out[f"{name}_ms"] = round(ms, 4)
                    want = g32.search(q, k)[1]
                    for name in ("fp16",) + tuple(n for g in first for n in (g, f"{g}_refined")) + ("binary_asym", "binary_asym_refined"):
                        out[f"{name}_recall_at_{k}"] = round(M.rank._recall(variants[name]()[1], want, k)[0], 4)
                    # each ratio: how many times faster the asymmetric search is than the other (above 1: faster)
                    out["binary_asym_vs_binary"] = round(med["binary"] / med["binary_asym"], 3)
                    out["binary_asym_vs_int8"] = round(med["int8"] / med["binary_asym"], 3)
                    out["binary_asym_shortlist_vs_binary_shortlist"] = round(med["binary_shortlist"] / med["binary_asym_shortlist"], 3)
                    out["binary_asym_refined_vs_binary_refined"] = round(med["binary_refined"] / med["binary_asym_refined"], 3)
                    out["binary_asym_refined_vs_int8_refined"] = round(med["int8_refined"] / med["binary_asym_refined"], 3)
                    for other in ("int8", f"pq{a.M}"):
                        out[f"binary_vs_{other}"] = round(med[other] / med["binary"], 3)
                        out[f"binary_refined_vs_{other}_refined"] = round(med[f"{other}_refined"] / med["binary_refined"], 3)
                    emit(out)
            del g32, g16, g8, pq, bg, variants, first
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
