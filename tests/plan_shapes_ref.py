"""Cases, slice metric, noise floor and modelled bugs for the conv backbones run block by block away from 224 x 224
(tests/test_plan_shapes_gpu.py compares every block with the oracle on the GPU, tests/test_plan_shapes_args.py checks the
table, the plans and the metric on the CPU).

What is under test is the executor, not a kernel: `resolve_plan`, `op_shape`, the arena slots, `run_backbone`'s marshalling and
`launch_gemm_bf16`'s dispatch on M = B * h * w.  The kernels have float64 tests of their own; here every block of a model runs
alone on the oracle's tap (`mi355_model_run_between_taps`) at input sizes whose maps are odd and non-square and at the batch
sizes on both sides of every dispatch edge, and is compared with the oracle's next tap over the whole tensor AND over slices
of it (rows, columns, groups of 8 channels): a slot one row short, a squeeze over the wrong count or a stride-2 phase on the
wrong side moves one slice a lot and the whole tensor little.

    python tests/plan_shapes_ref.py        prints the noise floor per (model, size) that N0 below records
"""
import functools
import os
import sys

import torch

if __name__ == "__main__":          # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch.nn.functional as F

from oracle import effnet, rexnet
from oracle.common import Rounder
from test_effnet_gpu import images

# ---------------------------------------------------------------------------------------------------------------- cases
MODELS = {"efficientnet_b3a": None, "rexnet_100": 1.0, "rexnet_130": 1.3, "rexnet_150": 1.5, "rexnet_200": 2.0}   # -> width
# (225, 231): 113x116 / 57x58 / 29 / 15 / 8 maps; split-K edge at 14x14-class maps (83 / 84), fuse_block_min_batch (95 / 96 / 97),
# 1024 rows at the last stage (21).  (32, 32): M = B in the last stage, so the 64 / 65 and 1023 / 1024 / 1025 row edges.
# (160, 224), (288, 224): W = 7 / 14 maps with H != W (whole-block kernel on the models' own channels); (256, 320) with the
# two above: the launch-plan golden's sizes; (300, 300): B3's native resolution, 150 / 75 / 38 / 19 / 10.
LADDERS = {
    (225, 231): (1, 2, 21, 83, 84, 95, 96, 97, 256),
    (32, 32): (1, 64, 65, 1023, 1024, 1025),
    (224, 224): (1, 21, 83, 84, 95, 97),            # 2 and 256: test_each_block_on_the_oracles_own_input
    (160, 224): (2, 96, 256),
    (288, 224): (2, 96, 256),
    (256, 320): (2, 96, 256),
    (300, 300): (2, 96, 256),
}
# rexnet_100 / 130 / 150 keep three sizes (the file's run time): 200 is the widest and the benchmark's, the three narrower ones
# differ from it in channel counts only, which the sizes kept here reach on even, odd and non-square maps.
TRIMMED = {"rexnet_100", "rexnet_130", "rexnet_150"}
TRIMMED_SIZES = ((224, 224), (225, 231), (160, 224))
POOLED_B = (2, 96)          # batch sizes of the pooled-path test, per (model, size)


def sizes(model):
    return [s for s in LADDERS if model not in TRIMMED or s in TRIMMED_SIZES]


def cases(model):
    return [(H, W, B) for (H, W) in sizes(model) for B in LADDERS[(H, W)]]


ALL_CASES = [(m, H, W, B) for m in MODELS for (H, W, B) in cases(m)]
ALL_SIZES = [(m, H, W) for m in MODELS for (H, W) in sizes(m)]


def family(model):
    return "effnet" if MODELS[model] is None else "rexnet"


TOL_BLOCK_ISOLATED = {"effnet": 1.5e-3, "rexnet": 2e-3}      # tests/test_effnet_gpu.py, tests/test_rexnet_gpu.py
TOL_EMB_SIM = 1e-2                                           # tests/test_effnet_gpu.py
IMAGE_SEED = {"effnet": 19, "rexnet": 23}                    # as the isolated-block tests at 224


# --------------------------------------------------------------------------------------------------------------- oracle
# With the seeded init the SE gate hardly depends on what it squeezes: d ln(block output) / d ln(squeeze) is about 0.1, so a
# squeeze over the wrong pixel count, or another image's gate, would move a block's output by less than its rounding bound.  Both
# SE matrices are therefore scaled by 4 here (the gates spread over most of (0, 1) without saturating), for the oracle and the
# model alike; everything else is the state dict of the isolated-block tests at 224.  That is for blocks run ALONE: through
# the whole network such gates amplify every rounding flip (the oracle's own fp32 and float64 embeddings then differ by 0.25 in
# relative L2 against 1.6e-3 with the plain weights), so the pooled-path test keeps the plain state dict (sharpen=False).
SE_SHARPEN = 4.0
_SE_MATRICES = ("se.conv_reduce.weight", "se.conv_expand.weight", "se.fc1.weight", "se.fc2.weight")


@functools.lru_cache(maxsize=None)
def state_dict(model, sharpen=True):
    sd = effnet.init_state_dict(2) if MODELS[model] is None else rexnet.init_state_dict(4, MODELS[model])
    for k in sd:
        if sharpen and k.endswith(_SE_MATRICES):
            sd[k] = sd[k] * SE_SHARPEN
    return sd


def layers(model, sharpen=True):
    """[(tap name, block dict or None, f(x, rb, hooks=None))], the stem first and the head last."""
    sd = state_dict(model, sharpen)
    return effnet.layers(sd) if MODELS[model] is None else rexnet.layers(sd, MODELS[model])


def oracle_taps(model, H, W, sharpen=True):
    """{tap: (2, C, h, w) fp32} of the sim_bf16 oracle on images(seed, 2, H, W), "head" included, in network order."""
    x = torch.from_numpy(images(IMAGE_SEED[family(model)], 2, H, W))
    rb = Rounder(True)
    taps = {}
    for name, _, f in layers(model, sharpen):
        x = f(x, rb)
        taps[name] = x
    return taps


def pool(fm):
    return fm.mean((2, 3))


def has_se(model, b):
    return True if family(model) == "effnet" else b["rd"] > 0


def partial_residual(model, b):
    return family(model) == "rexnet" and b["s"] == 1 and b["cin"] < b["cout"]


# -------------------------------------------------------------------------------------------------------- slice metric
MIN_SLICE = 4096


def _groups(n, per, min_elems=MIN_SLICE):
    """Index of the merged slice each of n rows (columns, channel groups) of `per` elements belongs to: neighbours are merged
    until a slice has at least `min_elems` elements, and a shorter remainder joins the last slice."""
    m = max(1, -(-min_elems // per))
    ng = max(1, n // m)
    return torch.clamp(torch.arange(n) // m, max=ng - 1), ng


def slice_worst(G, R, tol_floor=0.25):
    """G, R (B, C, H, W) on one device -> float64 tensor [whole, rows, columns, channel groups] of the worst
    ||G_S - R_S|| / max(||R_S||, 0.25 rms(R) sqrt(|S|)) over the slices S of each kind (whole: the project's rel L2).

    Rows: one output row y over images, channels and x; columns likewise; channel groups: 8 consecutive channels over images
    and pixels.  Neighbouring slices are merged until each holds MIN_SLICE elements (small maps: up to the whole tensor), so
    that a slice's own rounding noise stays a fraction of the whole tensor's bound."""
    G, R = G.double(), R.double()
    B, C, H, W = R.shape
    E, Q = (G - R) ** 2, R * R
    ms = Q.sum() / R.numel()
    out = [torch.sqrt(E.sum()) / (torch.sqrt(Q.sum()) + 1e-12)]
    cg = (C + 7) // 8
    chan_cnt = torch.full((cg,), 8.0 * B * H * W, dtype=torch.float64)
    chan_cnt[-1] = (C - 8 * (cg - 1)) * B * H * W
    for dims, n, per, first in (((0, 1, 3), H, B * C * W, None), ((0, 1, 2), W, B * C * H, None),
                                ((0, 2, 3), C, 8 * B * H * W, torch.arange(C) // 8)):
        e, q = E.sum(dims), Q.sum(dims)
        if first is not None:                # channels -> groups of 8 first (the last group may be narrower)
            e = torch.zeros(cg, dtype=e.dtype, device=e.device).index_add_(0, first.to(e.device), e)
            q = torch.zeros(cg, dtype=q.dtype, device=q.device).index_add_(0, first.to(q.device), q)
            cnt, n = chan_cnt, cg
        else:
            cnt = torch.full((n,), float(per), dtype=torch.float64)
        idx, ng = _groups(n, per)
        idx = idx.to(e.device)
        z = lambda: torch.zeros(ng, dtype=torch.float64, device=e.device)
        eg, qg, ng_cnt = z().index_add_(0, idx, e), z().index_add_(0, idx, q), z().index_add_(0, idx, cnt.to(e.device))
        den = torch.maximum(torch.sqrt(qg), tol_floor * torch.sqrt(ms * ng_cnt))
        out.append((torch.sqrt(eg) / den).max())
    return torch.stack(out)


# --------------------------------------------------------------------------------------------------------- noise floor
def noise_floor(model, H, W, taps=None):
    """The oracle's own flip noise: every layer behind the stem evaluated on the oracle's (bf16-rounded) previous tap twice,
    in fp32 as the oracle does and with the arithmetic between the same rounding points in float64.  The two differ only where
    a sum falls on the other side of a bf16 rounding boundary, which any correct kernel may do as well.
    -> {tap: float64 [whole, rows, columns, channel groups]}"""
    taps = taps or oracle_taps(model, H, W)
    rb = Rounder(True)
    out, prev = {}, None
    for name, _, f in layers(model):
        if prev is not None:
            out[name] = slice_worst(taps[name], f(taps[prev].double(), rb))
        prev = name
    return out


# Worst slice value of noise_floor over every (model, size) of the table, per family (printed by this file run as a script;
# tests/test_plan_shapes_args.py re-measures it).  SLICE_TOL = max(TOL_BLOCK_ISOLATED, 4 * N0): a factor 2 because a kernel has
# two independent flip sources inside a block (the expanded tensor E and the gated tensor A') where the fp32 / float64 pair
# exercises each once, and a factor 2 as margin.
N0 = {"effnet": 1.17e-3, "rexnet": 6.14e-4}


def slice_tol(model):
    fam = family(model)
    return max(TOL_BLOCK_ISOLATED[fam], 4.0 * N0[fam])


# -------------------------------------------------------------------------------------------------------- modelled bugs
def _shift_phase(x):
    """the stride-2 window one pixel further down / right: what padding on the other side gives"""
    return F.pad(x[..., 1:, 1:], (0, 1, 0, 1))


def _squeeze_padded_input_count(d):
    """a stride-2 block's squeeze divided by the pixel count of its INPUT map with the rows padded to even, ceil(H / 2) * 2 * W
    (W = 2 Wo or 2 Wo - 1; the even one is taken), where Ho * Wo is due"""
    Ho, Wo = d.shape[2:]
    return d.sum((2, 3), keepdim=True) / (Ho * 2 * Wo * 2)


def _squeeze_no_last_row(d):
    Ho, Wo = d.shape[2:]
    return d[:, :, :-1].sum((2, 3), keepdim=True) / (Ho * Wo)


def _residual_everywhere(x, sc, cin):
    return x + sc[:, torch.arange(x.shape[1]) % cin]


def _last_row_from_above(y):
    y = y.clone()
    y[:, :, -1] = y[:, :, -2]
    return y


def _last_col_replicated(y):
    y = y.clone()
    y[..., -1] = y[..., -2]
    return y


def _last8_zero(y):
    y = y.clone()
    y[:, -8:] = 0
    return y


# name -> (hooks planted in the block or None, map of the oracle's output tap or None, applies(model, block dict, out shape))
# `b` is None for the head conv, which only the output bugs reach.
MUTANTS = {
    "stride2_phase_shifted": ({"dw_in": _shift_phase}, None, lambda m, b, o: b is not None and b["s"] == 2),
    "last_row_from_the_row_above": (None, _last_row_from_above, lambda m, b, o: o[2] >= 2),
    "last_column_replicated": (None, _last_col_replicated, lambda m, b, o: o[3] >= 2),
    "squeeze_over_input_pixel_count": ({"squeeze": _squeeze_padded_input_count}, None,
                                       lambda m, b, o: b is not None and has_se(m, b) and b["s"] == 2),
    "squeeze_drops_last_row": ({"squeeze": _squeeze_no_last_row}, None, lambda m, b, o: b is not None and has_se(m, b)),
    "last_8_channels_zero": (None, _last8_zero, lambda m, b, o: True),
    "residual_on_every_column": ({"residual": _residual_everywhere}, None, lambda m, b, o: b is not None and partial_residual(m, b)),
    "gate_from_neighbour_image": ({"gate": lambda g: g.flip(0)}, None, lambda m, b, o: b is not None and has_se(m, b)),
}


def mutant_moves(model, H, W, taps=None):
    """{mutant: {tap: worst slice ratio (max over the three slice kinds and the whole tensor) of the bugged block against the
    oracle's tap}} for every layer the mutant applies to."""
    taps = taps or oracle_taps(model, H, W)
    rb = Rounder(True)
    out = {k: {} for k in MUTANTS}
    prev = None
    for name, b, f in layers(model):
        if prev is not None:
            R = taps[name]
            for mut, (hooks, post, applies) in MUTANTS.items():
                if applies(model, b, tuple(R.shape)):
                    bad = f(taps[prev], rb, hooks) if hooks else post(R)
                    out[mut][name] = float(slice_worst(bad, R).max())
        prev = name
    return out


if __name__ == "__main__":
    worst = {}
    for model, H, W in ALL_SIZES:
        nf = noise_floor(model, H, W)
        w = torch.stack(list(nf.values())).max(0).values
        at = max(nf, key=lambda k: float(nf[k][1:].max()))
        print(f"{model:18s} {H}x{W}: whole {w[0]:.3e} rows {w[1]:.3e} cols {w[2]:.3e} chan {w[3]:.3e}  (worst slice at {at})", flush=True)
        worst[family(model)] = max(worst.get(family(model), 0.0), float(w[1:].max()))
    print("N0 =", worst)
    sys.exit(0)
