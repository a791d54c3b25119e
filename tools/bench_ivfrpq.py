"""Search time, size, quantisation error and recall of the residual IVF-PQ index (developer tool): ``ResidualIVFPQIndex.search``
against ``IVFPQIndex.search`` (the code of before the residual index, untouched) over the same rows, the same k-means lists and
the same queries.  The two run in alternation in one process, each rep timed with HIP events around ``--calls`` back-to-back
searches, after a warm-up of both; the median of the reps is reported, one JSON line per (rows, G, M, nprobe, Q, k) cell with
both times, their ratio, and recall@k against the fp32 gallery's search - raw, and with ``refine=`` the fp32 gallery - for both;
and one line per index with its build time, its bytes and ``mean |rn - reconstruct|^2``.

    python tools/bench_ivfrpq.py [--rows clusters,normal] [--G 100000,1000000] [--Q 1,16,256] [--k 3,150] [--M 48,96]
                                 [--nlist 1024] [--nprobe 1,8,32] [--train-rows 100000] [--pq-iters 10] [--iters 10]
                                 [--reps 9] [--calls 5] [--shortlist 100] [--out profiles/ivfrpq_bench.txt]

Both indexes train their codebooks on ``--train-rows`` rows (the plain one on the first rows, the residual one on the rows
``seeded_rows`` picks; the rows are independent draws, so either is a random sample) and share the lists: the k-means of the
fp32 gallery with the same seed.  The refined search takes a shortlist of ``--shortlist`` rows, or k where k is larger.  Both
searches read one flag word back at the end of every call.  Rows as in tools/bench_pq.py.
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


def _mse(g32, recon):
    """mean |rn - reconstruct|^2 over the gallery's rows, float64 sums, in blocks."""
    total = 0.0
    for a in range(0, len(g32), 1 << 16):
        d = (g32.data[a: a + (1 << 16)] - recon[a: a + (1 << 16)]).double()
        total += float((d * d).sum())
    return total / len(g32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="clusters,normal")
    ap.add_argument("--G", default="100000,1000000")
    ap.add_argument("--Q", default="1,16,256")
    ap.add_argument("--k", default="3,150")
    ap.add_argument("--M", default="48,96")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", default="1,8,32")
    ap.add_argument("--train-rows", type=int, default=100000)
    ap.add_argument("--pq-iters", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shortlist", type=int, default=100)
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
            n_train = min(G, a.train_rows)
            g32.kmeans(8, iters=1)                                   # warm-up of the clustering kernels
            warm = M.PQGallery(D, dev, 96).train(x[:1024], iters=1).add(x[:1024])       # ... and of the PQ kernels
            M.ResidualIVFPQIndex.build(x[:1024], 96, 8, iters=1, pq_iters=1)
            del warm
            torch.cuda.synchronize()
            pairs = {}
            for m in _ints(a.M):
                def plain_build():
                    g = M.PQGallery(D, dev, m, capacity=G).train(x[:n_train], iters=a.pq_iters).add(x)
                    return M.IVFPQIndex.build(g, g32, a.nlist, iters=a.iters)
                plain, plain_ms = _timed(plain_build)
                resid, resid_ms = _timed(lambda: M.ResidualIVFPQIndex.build(g32, m, a.nlist, iters=a.iters, pq_iters=a.pq_iters,
                                                                            train_rows=n_train))
                assert torch.equal(plain.assignments, resid.assignments)              # the same lists
                pairs[m] = (plain, resid)
                emit({"rows": kind, "G": G, "D": D, "M": m, "nlist": a.nlist, "iters": a.iters, "pq_iters": a.pq_iters,
                      "train_rows": n_train,
                      "ivfpq": {"build_ms": round(plain_ms, 1), "nbytes": plain.nbytes + plain.pq.nbytes,
                                "mse": round(_mse(g32, plain.pq.reconstruct()), 6)},
                      "ivfrpq": {"build_ms": round(resid_ms, 1), "nbytes": resid.nbytes,
                                 "mse": round(_mse(g32, resid.reconstruct()), 6)}})
            del x
            for Q in _ints(a.Q):
                q = _rows(Q, 13, kind, dev)
                for k in _ints(a.k):
                    exact = g32.search(q, k)[1]
                    short = max(a.shortlist, k)
                    for m, (plain, resid) in pairs.items():
                        for nprobe in _ints(a.nprobe):
                            variants = {"ivfpq": lambda: plain.search(q, k, nprobe), "ivfrpq": lambda: resid.search(q, k, nprobe)}
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
                            med = {name: statistics.median(v) for name, v in times.items()}
                            out = {"rows": kind, "G": G, "D": D, "M": m, "nlist": a.nlist, "nprobe": nprobe, "Q": Q, "k": k,
                                   "reps": a.reps, "calls": a.calls, "shortlist": short,
                                   "ratio": round(med["ivfrpq"] / med["ivfpq"], 3)}
                            for name, ix in (("ivfpq", plain), ("ivfrpq", resid)):
                                raw = ix.search(q, k, nprobe)[1]
                                fine = ix.search(q, k, nprobe, refine=g32, shortlist=short)[1]
                                out[name] = {"ms": round(med[name], 4), "min_ms": round(min(times[name]), 4),
                                             "max_ms": round(max(times[name]), 4), f"recall_at_{k}": round(_recall(raw, exact), 4),
                                             f"refined_recall_at_{k}": round(_recall(fine, exact), 4)}
                            emit(out)
            del g32, pairs, variants, plain, resid
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
