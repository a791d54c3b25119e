"""The committed bench lines (profiles/rNN_bench_n1.json, produced by `python bench.py` on an MI355X) carry every field
of the driver's contract, and bench.py still emits those keys (static check of the source: no GPU here).  With a GPU,
a small bench run checks --steps / ms_per_step and that --dump-outputs writes what the timed path computed."""
import json
import os
import re

import numpy as np
import pytest

from helpers import ROOT

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]
ROOFLINE = ["bound", "achieved", "peak", "unit", "frac", "traffic"]
CPU = ["value", "unit", "cores", "kind", "sample"]


@pytest.mark.parametrize("name", ["r01_bench_n1.json", "r02_bench_n1.json", "r03_bench_n1.json"])
def test_committed_bench_line_has_the_contract_fields(name):
    line = open(os.path.join(ROOT, "profiles", name)).read().strip().splitlines()[-1]
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    for k in ROOFLINE:
        assert k in d["roofline"], k
    for k in CPU:
        assert k in d["cpu_baseline"], k
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["roofline"]["bound"] in ("hbm", "mfma") and 0.0 < d["roofline"]["frac"] < 1.0
    assert abs(d["roofline"]["frac"] - d["roofline"]["achieved"] / d["roofline"]["peak"]) < 1e-9
    assert d["cpu_baseline"]["kind"] in ("port", "reference") and d["cpu_baseline"]["cores"] >= 1
    assert "workload" in d["config"] and "model" not in d["config"]
    if not name.startswith("r01"):
        assert d["roofline"]["traffic"] and d["roofline"]["launches_per_forward"] >= 1   # PMC traffic of the same sources
    # value = images of all ranks / time of the timed steps
    assert abs(d["value"] - d["config"]["batch_per_gpu"] * d["n_gpus"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


def test_bench_source_still_emits_the_contract_keys():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for k in REQUIRED:
        assert re.search(rf'"{k}"', src), k
    assert "/root/reference" not in src
    assert "--dump-outputs" in src


@pytest.mark.gpu
def test_bench_dump_outputs_hold_the_timed_paths_top_k(tmp_path):
    """bench.py in a fresh child process on a small batch / gallery: the JSON line reports the steps asked for, and
    DIR/*.npy equal, bit for bit, the top-k that the same seeded model, images and gallery give in this process."""
    import subprocess
    import sys
    import torch
    import imageretrievalresearch_amd as M
    from imageretrievalresearch_amd import synth
    B, G, D, K = 16, 5000, 1536, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
           "--gallery", str(G), "--no-cpu-baseline", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    v = np.load(tmp_path / "topk_values.npy")
    i = np.load(tmp_path / "topk_indices.npy")
    assert v.dtype == np.float32 and i.dtype == np.float64 and v.shape == i.shape == (B, K)

    dev = torch.device("cuda", 0)
    model = M.create_model("efficientnet_b3a", num_classes=0, seed=0).to(dev).eval()
    x = M.synth_fill(B * 3 * 224 * 224, 1000, synth.UNIFORM, dev).view(B, 3, 224, 224)
    gal = M.ShardedGallery(M.synth_fill(G * D, 5, synth.NORMAL, dev).view(G, D))
    wv, wi = gal.search(model(x), K)
    np.testing.assert_array_equal(v, wv.cpu().numpy())
    np.testing.assert_array_equal(i, wi.cpu().numpy().astype(np.float64))
