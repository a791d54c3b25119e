"""Result diversification timings (developer tool).  One JSON line per gallery dtype; per (queries Q, shortlist L), k = 10, in ms:

* ``search``: the shortlist search alone (``rerank._shortlist_search``, what ``diversify`` starts with);
* ``gram`` / ``select``: ``mi355_shortlist_gram`` and ``mi355_mmr_select`` alone on a shortlist made beforehand, the Gram matrices in
  blocks of at most 256 MiB as ``diversify`` holds them;
* ``diversify``: ``Gallery.diversify(q, 10, lam=0.7, shortlist=L)`` end to end, and ``added`` = diversify - search;
* ``torch_gram`` / ``torch_select``: what a user would write in torch on the same shortlist - gather the fp16 rows (an fp16 copy
  of the gallery made beforehand), ``torch.bmm`` to fp32, and a k-step loop of torch ops - and ``torch_added``, their sum.

All variants in alternation in one process, HIP events around ``--calls`` back-to-back calls, median of ``--reps`` after warm-up.
Clustered synthetic rows, those of tools/bench_diffusion.py.

    python tools/bench_diversify.py [--dtypes fp32 fp16] [--dim 1536] [--rows 100000] [--out profiles/diversify_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import diversify as D  # noqa: E402
from imageretrievalresearch_amd import rerank as K  # noqa: E402


def _time(variants, reps, calls):
    for fn in variants.values():
        for _ in range(2):
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
    return {name: round(statistics.median(v), 3) for name, v in times.items()}


def _torch_gram(rows16, si):
    x = rows16[si.clamp_min(0)]                                      # (Q, L, D) fp16
    return torch.bmm(x, x.transpose(1, 2)).float()


def _torch_select(sv, si, S, k, lam):
    Q, L = si.shape
    m = torch.zeros_like(sv)
    free = si >= 0
    rows = torch.arange(Q, device=si.device)
    out = []
    for _ in range(k):
        v = torch.where(free, lam * sv - (1 - lam) * m, float("-inf"))
        j = v.argmax(dim=1)
        out.append(j)
        free[rows, j] = False
        m = torch.maximum(m, S[rows, j])
    pos = torch.stack(out, 1)
    return torch.gather(sv, 1, pos), torch.gather(si, 1, pos)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", choices=("fp32", "fp16"), nargs="+", default=["fp32", "fp16"])
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--queries", type=int, nargs="+", default=[256, 1])
    ap.add_argument("--shortlists", type=int, nargs="+", default=[100, 200, 1024])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_diversify.py measures on the GPU: there is no CPU path"
    dev = "cuda:0"
    G, Dm, Qmax = a.rows, a.dim, max(a.queries)
    gen = torch.Generator(device=dev).manual_seed(1)
    centers = torch.randn(1000, Dm, device=dev, generator=gen)
    lab = torch.randint(0, 1000, (G + Qmax,), device=dev, generator=gen)
    x = centers[lab] + a.spread * torch.randn(G + Qmax, Dm, device=dev, generator=gen)
    for dtype in a.dtypes:
        gal = M.Gallery(Dm, dev, dtype=torch.float16 if dtype == "fp16" else torch.float32).add(x[:G])
        rows16 = gal.data.half().contiguous()
        result = {}
        for Q in a.queries:
            q = x[G: G + Q].contiguous()
            for L in a.shortlists:
                sv, si = K._shortlist_search(gal, q, L, None)
                sv, si = sv.contiguous(), si.contiguous()
                block = D.diversify_params(G, a.k, a.lam, None, L)[4]
                scratch = torch.empty((min(block, Q), L, L), dtype=torch.float32, device=dev)

                def gram():
                    for q0 in range(0, Q, block):
                        D._dv_gram(gal, si[q0: q0 + block], scratch[: min(block, Q - q0)])

                def select():                                    # on what gram() left (past one block: the last block's, timing only)
                    for q0 in range(0, Q, block):
                        n = min(block, Q - q0)
                        D._dv_select(sv[q0: q0 + n], si[q0: q0 + n], scratch[:n], a.k, a.lam)

                St = _torch_gram(rows16, si)
                t = _time({"search": lambda: K._shortlist_search(gal, q, L, None), "gram": gram, "select": select,
                           "diversify": lambda: gal.diversify(q, a.k, lam=a.lam, shortlist=L),
                           "torch_gram": lambda: _torch_gram(rows16, si),
                           "torch_select": lambda: _torch_select(sv, si, St, a.k, a.lam)}, a.reps, a.calls)
                t["added"] = round(t["diversify"] - t["search"], 3)
                t["torch_added"] = round(t["torch_gram"] + t["torch_select"], 3)
                same = torch.equal(gal.diversify(q, a.k, lam=a.lam, shortlist=L)[1], _torch_select(sv, si, St, a.k, a.lam)[1])
                t["torch_picks_equal"] = bool(same)
                result[f"Q{Q}_L{L}"] = t
                del St, scratch
        line = json.dumps({"case": "diversify", "rows": G, "dim": Dm, "dtype": dtype, "k": a.k, "lam": a.lam, "ms": result})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del gal, rows16


if __name__ == "__main__":
    main()
