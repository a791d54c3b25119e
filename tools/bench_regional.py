"""Regional MaxSim re-ranking timings (developer tool).  One JSON line per shape (rows, R, Rq, dim, shortlist L, queries Q):

* ``scores_ms``: ``RegionGallery.scores(q, idx)`` on a shortlist made beforehand (the query codes and the score kernel);
  ``kernel_ms``: ``mi355_region_scores`` alone on codes made beforehand;
* ``rerank_ms``: ``RegionGallery.rerank(gallery, queries, q, 10, shortlist=L)``, its global shortlist search included, and
  ``search_ms``: that shortlist search alone;
* ``torch_ms``: the same arithmetic as a user would write it in torch on the same fp16 codes - ``g[idx]`` gather, ``einsum``,
  ``amax``, weighted sum - and ``max_diff`` between its scores and the kernel's;
* ``candidate_bytes`` = Q * L * R * ld * 2, ``gbs`` = that over ``kernel_ms``, and ``copy_share`` = ``gbs`` over ``copy_gbs``, the rate
  of a 1 GiB device copy (bytes read + written, as tools/bw.py counts them) measured in the same run: how far the kernel is
  from the floor of its gather.

All variants of a shape run in alternation in one process, HIP events around ``--calls`` back-to-back calls, median of ``--reps``
after warm-up.  Random unit regions; the global gallery is ``pooled()``.

    python tools/bench_regional.py [--rows 100000] [--out profiles/regional_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd import rerank as K  # noqa: E402
from imageretrievalresearch_amd._lib import check, lib, stream_ptr  # noqa: E402


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
    return {name: round(statistics.median(v), 4) for name, v in times.items()}


def _copy_gbs(dev):
    a = torch.empty(1 << 29, dtype=torch.bfloat16, device=dev).normal_()
    b = torch.empty_like(a)
    ms = _time({"copy": lambda: b.copy_(a)}, 7, 10)["copy"]
    return 2 * a.numel() * 2 / (ms * 1e-3) / 1e9


def _gallery(rows, R, dim, dev, gen, block=8192):
    rg = M.RegionGallery(dim, R, dev, capacity=rows)
    for r0 in range(0, rows, block):
        rg.add(torch.randn(min(block, rows - r0), R, dim, device=dev, generator=gen))
    return rg


def _torch_scores(qc, g, idx, w):
    c = g[idx]                                                   # (Q, L, R, ld) fp16: the gather
    s = torch.einsum("qid,qljd->qlij", qc, c)                    # fp16 in, fp32 accumulation inside, fp16 out
    return (s.float().amax(dim=3) * w[:, None, :]).sum(dim=2)


def _cell(rg, gal, Q, Rq, L, dev, gen, a):
    rows, R, dim, ld = rg.rows, rg.regions, rg.dim, rg._ld
    pick = torch.randint(0, rows, (Q,), device=dev, generator=gen)
    q = rg.data[pick][:, torch.arange(Rq, device=dev) % R].float() + 0.5 * torch.randn(Q, Rq, dim, device=dev, generator=gen) / dim ** 0.5
    qg = M.RegionGallery(dim, Rq, dev).add(q).pooled().data.contiguous()
    idx = K._shortlist_search(gal, qg, L, None)[1].contiguous()
    qc = rg.query_codes(q)
    out = torch.empty((Q, L), dtype=torch.float32, device=dev)
    w = torch.full((Q, Rq), 1.0 / Rq, device=dev)

    def kernel():
        check(lib().mi355_region_scores(qc.data_ptr(), Q, Rq, rg._buf.data_ptr(), rows, R, dim, ld, idx.data_ptr(), L, None,
                                        out.data_ptr(), None, stream_ptr(dev)))
    variants = {"kernel_ms": kernel, "scores_ms": lambda: rg.scores(q, idx), "search_ms": lambda: K._shortlist_search(gal, qg, L, None),
                "rerank_ms": lambda: rg.rerank(gal, qg, q, 10, shortlist=L)}
    g = rg._buf[:rows]
    if not a.no_torch:
        variants["torch_ms"] = lambda: _torch_scores(qc, g, idx, w)
    t = _time(variants, a.reps, a.calls)
    diff = None if a.no_torch else round(float((_torch_scores(qc, g, idx, w) - rg.scores(q, idx)).abs().max()), 6)
    nbytes = Q * L * R * ld * 2
    gbs = nbytes / (t["kernel_ms"] * 1e-3) / 1e9
    return {"case": "regional", "rows": rows, "R": R, "Rq": Rq, "dim": dim, "L": L, "Q": Q, **t, "torch_max_diff": diff,
            "candidate_bytes": nbytes, "gflop": round(2.0 * Q * L * R * Rq * dim / 1e9, 2), "gbs": round(gbs, 1),
            "copy_gbs": round(a.copy_gbs, 1), "copy_share": round(gbs / a.copy_gbs, 3),
            "lds_bytes": int(lib().mi355_region_scores_lds_bytes(Rq, dim))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--regions", type=int, default=14)
    ap.add_argument("--dims", type=int, nargs="+", default=[1536, 256])
    ap.add_argument("--shortlists", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--wide-rows", type=int, default=20000, help="rows of the one R = Rq = 64 cell (dim 1536, L = 100, Q = 256); 0: skip")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_regional.py measures on the GPU: there is no CPU path"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    a.copy_gbs = _copy_gbs(dev)
    lines = []

    def emit(cell):
        line = json.dumps(cell)
        print(line, flush=True)
        lines.append(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for dim in a.dims:
        rg = _gallery(a.rows, a.regions, dim, dev, gen)
        gal = rg.pooled(torch.float16)
        for L in a.shortlists:
            for Q in a.queries:
                emit(_cell(rg, gal, Q, a.regions, min(L, a.rows), dev, gen, a))
        del rg, gal
        torch.cuda.empty_cache()
    if a.wide_rows:
        rg = _gallery(a.wide_rows, 64, 1536, dev, gen, block=2048)
        emit(_cell(rg, rg.pooled(torch.float16), 256, 64, 100, dev, gen, a))


if __name__ == "__main__":
    main()
