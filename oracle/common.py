"""Shared helpers for the backbone oracles (TEST INFRASTRUCTURE — see oracle/__init__.py)."""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

from imageretrievalresearch_amd import synth  # data generator only (no compute path)


def make_divisible(v, divisor=8, min_value=None, round_limit=0.9):
    """timm 0.4.12 ``make_divisible`` (models/layers/helpers.py): channel rounding."""
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


class Rounder:
    """bf16 rounding points of the HIP path.  ``sim=False`` -> identity (pure fp32 = the
    reference's CPU semantics, autocast is a no-op without CUDA: inference/inference.py:196).  The dtype of ``x`` is kept: a
    float64 activation is rounded to bf16 at the same points and comes back as float64, so an oracle fed a float64 tensor
    keeps its rounding points and does the arithmetic between them in float64 (tests/plan_shapes_ref.py measures the
    fp32 oracle's own rounding-flip noise that way)."""

    def __init__(self, sim: bool):
        self.sim = sim

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return x.to(torch.bfloat16).to(x.dtype) if self.sim else x


def bn_scale(bn: dict, eps: float) -> torch.Tensor:
    """g / sqrt(v + eps) in fp32 with a correctly rounded square root, as the packer's sqrtf.  (torch.sqrt of an fp32
    tensor on CPU can be one ulp off; the float64 root rounded to fp32 is the correctly rounded fp32 root.)"""
    v = bn["running_var"] + eps
    return bn["weight"] / torch.sqrt(v.double()).to(v.dtype)


def fold_bn(w: torch.Tensor, bn: dict, eps: float, dtype=None):
    """conv weight (O, ...) + eval-mode BN -> (w * g/sqrt(v+eps), b - m*g/sqrt(v+eps)).  The fold is the packer's, in fp32
    whatever ``dtype`` says; ``dtype`` only converts the two results (exactly) for a conv on an activation of that dtype."""
    scale = bn_scale(bn, eps)
    shape = [-1] + [1] * (w.dim() - 1)
    wf, bf = w * scale.reshape(shape), bn["bias"] - bn["running_mean"] * scale
    return (wf, bf) if dtype is None else (wf.to(dtype), bf.to(dtype))


def bn_of(sd, prefix):
    return {k: sd[f"{prefix}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")}


class SeededInit:
    """Seeded random-init weights (SURVEY §8d cfg 1): conv/linear N(0, 2/fan_in), BN gamma
    U[0.5,1.5], beta N(0,0.1), running_mean N(0,0.1), running_var U[0.5,1.5].  Each tensor is
    its own stream ``seed*100003 + ordinal`` of the portable generator, so the same state dict
    can be rebuilt anywhere without torch RNG."""

    def __init__(self, seed: int):
        self.seed = seed
        self.n = 0
        self.sd = OrderedDict()

    def _next(self):
        self.n += 1
        return self.seed * 100003 + self.n

    def conv(self, name, shape, fan_in=None, gain=2.0):
        fan_in = fan_in or int(np.prod(shape[1:]))
        w = synth.normal(self._next(), shape) * np.float32(math.sqrt(gain / fan_in))
        self.sd[name] = torch.from_numpy(w.astype(np.float32))

    def vec(self, name, n, kind, lo=0.0, scale=1.0):
        if kind == "normal":
            v = synth.normal(self._next(), (n,)) * np.float32(scale) + np.float32(lo)
        else:
            v = synth.uniform(self._next(), (n,)) * np.float32(scale) + np.float32(lo)
        self.sd[name] = torch.from_numpy(v.astype(np.float32))

    def bn(self, prefix, n):
        self.vec(f"{prefix}.weight", n, "uniform", 0.5, 1.0)
        self.vec(f"{prefix}.bias", n, "normal", 0.0, 0.1)
        self.vec(f"{prefix}.running_mean", n, "normal", 0.0, 0.1)
        self.vec(f"{prefix}.running_var", n, "uniform", 0.5, 1.0)
        self.sd[f"{prefix}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)

    def ln(self, prefix, n):
        self.vec(f"{prefix}.weight", n, "uniform", 0.5, 1.0)
        self.vec(f"{prefix}.bias", n, "normal", 0.0, 0.1)


def count_params(sd, include_buffers=False):
    tot = 0
    for k, v in sd.items():
        if not include_buffers and (k.endswith("running_mean") or k.endswith("running_var")
                                    or k.endswith("num_batches_tracked")
                                    or k.endswith("relative_position_index") or k.endswith("attn_mask")):
            continue
        tot += v.numel()
    return tot
