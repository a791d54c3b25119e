"""Feature-map aggregation timings (developer tool).  One JSON line per map shape, and per method in it:

* ``us``: one ``aggregate(fm, method)`` call, in microseconds;
* ``torch_us``: the composition of torch ops a user would write for the same descriptor on the same device (``TORCH`` below: for
  R-MAC one slice, reduction and normalisation per region), and its largest difference to ``aggregate``;
* ``x``: ``torch_us / us`` (below 1: the torch composition is not slower);
* ``copy_share``: the map's bytes (once, also for CroW, which reads it twice) over the call's time, as a share of the 6.29 TB/s
  copy rate of the MI355X;
* for ``spoc`` also ``pool_linear_us``, the library's existing mean-pool entry (no normalisation).

All variants of a shape in alternation in one process, HIP events around ``--calls`` back-to-back calls, median of ``--reps``
(after warm-up).  The times include the host's launches: the calls are microseconds long and the launch floor is most of them.

    python tools/bench_aggregate.py [--out profiles/aggregate_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import imageretrievalresearch_amd as M  # noqa: E402
from imageretrievalresearch_amd.models import pool_linear  # noqa: E402

COPY_RATE = 6.29e12
SHAPES = [(256, 1536, 7, 7), (256, 2560, 7, 7), (1, 1536, 7, 7), (32, 1536, 32, 32)]
EPS = 1e-6


def _l2(v):
    return v / v.norm(dim=-1, keepdim=True).clamp_min(EPS)


def _gem(x, p=3.0):
    return x.clamp(min=1e-6).pow(p).mean((2, 3)).pow(1.0 / p)


def _rmac(fm, regions, pool):
    out = 0
    for y, x, h, w in regions:
        out = out + _l2(pool(fm[:, :, y:y + h, x:x + w]))
    return _l2(out)


def _crow(fm):
    xp = fm.clamp(min=0)
    S = xp.sum(1, keepdim=True)
    z = S.pow(2).sum((2, 3), keepdim=True).sqrt()
    St = torch.where(z > 0, (S / z.clamp_min(1e-30)).sqrt(), torch.zeros_like(S))
    Fc = (St * xp).sum((2, 3))
    Q = (fm > 0).float().mean((2, 3))
    I = torch.where(Q > 0, (Q.sum(1, keepdim=True) / Q.clamp_min(1e-30)).log(), torch.zeros_like(Q))
    return _l2(I * Fc)


def _variants(fm):
    regions = M.rmac_regions(fm.shape[2], fm.shape[3]).tolist()
    ours = {"spoc": lambda: M.aggregate(fm, "spoc"), "mac": lambda: M.aggregate(fm, "mac"), "gem": lambda: M.aggregate(fm, "gem"),
            "rmac": lambda: M.aggregate(fm, "rmac"), "rmac_gem": lambda: M.aggregate(fm, "rmac", pool="gem"),
            "crow": lambda: M.aggregate(fm, "crow")}
    TORCH = {"spoc": lambda: _l2(fm.mean((2, 3))), "mac": lambda: _l2(fm.amax((2, 3))), "gem": lambda: _l2(_gem(fm)),
             "rmac": lambda: _rmac(fm, regions, lambda v: v.amax((2, 3))), "rmac_gem": lambda: _rmac(fm, regions, _gem),
             "crow": lambda: _crow(fm)}
    return ours, TORCH, len(regions)


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
            times[name].append(t0.elapsed_time(t1) / calls * 1e3)
    return {name: statistics.median(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aggregate.py measures on the GPU: there is no CPU path"
    dev = "cuda:0"
    for shape in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        fm = F.silu(2.0 * torch.randn(shape, device=dev, generator=gen))
        ours, TORCH, R = _variants(fm)
        variants = {**{f"ours/{k}": v for k, v in ours.items()}, **{f"torch/{k}": v for k, v in TORCH.items()},
                    "pool_linear": lambda: pool_linear(fm)}
        t = _time(variants, a.reps, a.calls)
        nbytes = fm.numel() * 4
        methods = {}
        for k in ours:
            us, tus = t[f"ours/{k}"], t[f"torch/{k}"]
            methods[k] = {"us": round(us, 1), "torch_us": round(tus, 1), "x": round(tus / us, 2),
                          "copy_share": round(nbytes / (us * 1e-6) / COPY_RATE, 3),
                          "max_diff_to_torch": float(f"{(ours[k]() - TORCH[k]()).abs().max().item():.2e}")}
        methods["spoc"]["pool_linear_us"] = round(t["pool_linear"], 1)
        line = json.dumps({"case": "aggregate", "shape": list(shape), "map_bytes": nbytes, "rmac_regions": R, "reps": a.reps,
                           "calls": a.calls, "methods": methods})
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
