"""Feature-map aggregation (not in the reference, whose only aggregation is the mean of ``get_fm``): how a backbone's last map
becomes the descriptor that ``Whitening``, query expansion and the re-rankers were evaluated on.

* ``spoc`` ... the mean over positions (Babenko and Lempitsky, ICCV 2015): ``pool_linear(fm)``'s arithmetic, here for completeness
* ``mac`` .... the maximum over positions (Tolias, Sicre and Jegou, ICLR 2016)
* ``gem`` .... generalised mean, ``(mean(max(x, 1e-6)^p))^(1/p)`` (Radenovic, Tolias and Chum, TPAMI 2018), p = 3 by default, a
               scalar or one value per channel, evaluated as ``m (mean((t/m)^p))^(1/p)`` so that no power overflows
* ``rmac`` ... the regional vectors of ``rmac_regions`` (max by default, ``pool="gem"`` or ``"mean"``), each normalised, summed and
               normalised again (Tolias et al.); with ``whitening=`` each regional vector is whitened before the sum
* ``crow`` ... cross-dimensional weighting with alpha = beta = 2 (Kalantidis, Mellina and Osindero, ECCV 2016)
* ``regions``  the caller's own (y0, x0, h, w) list instead of the R-MAC grid

One pass over the map in HBM for every method but CroW (two), every region pooled from LDS (csrc/aggregate.hip; the arithmetic
is stated in include/mi355_retrieval.h).  fp32 throughout, a fixed order of every sum: an image's descriptor is the same bits on
every run, at every batch size and at every position in the batch.  Nothing here reads a result back to the host.

Out of scope: fusing the aggregation into the head kernel (the fp32 map ``forward_features`` returns is read here); multi-scale
descriptors (there is no float-image resize: sum the descriptors of several input sizes and ``l2_normalize_rows`` them);
learning ``p`` (no backward)."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import MI355Error, check, lib, require_cuda, stream_ptr
from . import rank as _rank

MAX_SIDE, MAX_REGIONS, MAX_P = 64, 64, 64.0
EPS_CLAMP = 1e-6
METHODS = ("spoc", "mac", "gem", "rmac", "crow", "regions")
_POOLS = {"mean": 0, "max": 1, "gem": 2}
_PRESET = {"spoc": "mean", "mac": "max", "gem": "gem"}


def _side(name, v, lo=1, hi=MAX_SIDE) -> int:
    if not _rank._is_int(v) or not lo <= int(v) <= hi:
        raise MI355Error(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def rmac_regions(H: int, W: int, levels: int = 3, overlap: float = 0.4) -> torch.Tensor:
    """The R-MAC region grid of an H x W map: int32 (R, 4) rows (y0, x0, h, w) on the host.  With w = min(H, W): the longer side
    gets ``idx + 1`` extra steps, ``idx`` the first of s = 2..7 (counted from 0) that minimises ``|(w^2 - w b_s) / w^2 - overlap|``,
    ``b_s = (max(H, W) - w) / (s - 1)`` (float64); a square map gets none.  Level l = 1..levels has squares of side
    ``wl = floor(2 w / (l + 1))`` (skipped when 0) at ``floor(wl2 + i step) - wl2``, ``wl2 = floor(wl / 2 - 1)``, ``step = (S - wl) /
    (l + d - 1)`` along a side S with d extra steps - in integers, ``i (S - wl) // (l + d - 1)``.  Rows outer, columns inner, levels in
    order, duplicates kept.  7 x 7 gives 14 regions: the map, 4 x 4 at {0, 3}^2 and 3 x 3 at {0, 2, 4}^2."""
    H, W = _side("H", H), _side("W", W)
    levels = _side("levels", levels, 1, 8)
    try:
        overlap = float(overlap)
    except (TypeError, ValueError):
        raise MI355Error(f"overlap must be a float, got {overlap!r}") from None
    if not np.isfinite(overlap):
        raise MI355Error(f"overlap must be finite, got {overlap!r}")
    w = min(H, W)
    dH = dW = 0
    if H != W:
        cost = [abs((w * w - w * ((max(H, W) - w) / (s - 1))) / (w * w) - overlap) for s in range(2, 8)]
        d = cost.index(min(cost)) + 1
        dH, dW = (d, 0) if H > W else (0, d)
    out = []
    for l in range(1, levels + 1):
        wl = 2 * w // (l + 1)
        if wl == 0:
            continue

        def starts(S, n):
            return [0 if n == 1 else i * (S - wl) // (n - 1) for i in range(n)]
        for y in starts(H, l + dH):
            for x in starts(W, l + dW):
                out.append((y, x, wl, wl))
    return torch.tensor(out, dtype=torch.int32).reshape(-1, 4)


def _host_regions(regions, H: int, W: int) -> torch.Tensor:
    try:
        t = torch.as_tensor(regions).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise MI355Error(f"regions must be an integer (R, 4) list of (y0, x0, h, w), got {type(regions).__name__}") from None
    if t.dim() != 2 or t.shape[1] != 4 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise MI355Error(f"regions must be an integer (R, 4) list of (y0, x0, h, w), got {t.dtype} {tuple(t.shape)}")
    if not 1 <= t.shape[0] <= MAX_REGIONS:
        raise MI355Error(f"regions: R={t.shape[0]} outside [1, {MAX_REGIONS}]")
    t = t.to(torch.int64)
    y0, x0, h, w = t.unbind(1)
    bad = (h < 1) | (w < 1) | (y0 < 0) | (x0 < 0) | (y0 + h > H) | (x0 + w > W)
    if bool(bad.any()):
        r = int(torch.nonzero(bad)[0])
        raise MI355Error(f"regions: region {r} = {tuple(int(v) for v in t[r])} is empty or outside the {H}x{W} map")
    return t.to(torch.int32).contiguous()


def _p_arg(p, C: int, device):
    """(scalar p, device tensor or None) for the gem pool."""
    if torch.is_tensor(p) and p.dim() > 0:
        if p.dim() != 1 or p.shape[0] != C:
            raise MI355Error(f"a per-channel p must be a ({C},) tensor, got {tuple(p.shape)}")
        return 1.0, p.detach().to(device, torch.float32).contiguous()
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise MI355Error(f"p must be a float in (0, {MAX_P:g}] or a (C,) tensor, got {p!r}") from None
    if not np.isfinite(p) or not 0.0 < float(np.float32(p)) <= MAX_P:
        raise MI355Error(f"p must be a float in (0, {MAX_P:g}], got p={p!r}")
    return p, None


def _eps(eps) -> float:
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise MI355Error(f"eps must be a finite float >= 0, got {eps!r}") from None
    if not np.isfinite(eps) or eps < 0:
        raise MI355Error(f"eps must be a finite float >= 0, got {eps!r}")
    return eps


def _workspace(dev, B: int, C: int, R: int):
    return _rank._ws.get(dev, max(int(lib().mi355_aggregate_workspace_bytes(B, C, R)), 1))


def _pool_regions(fm, regs, pool: int, p, pvec, normalize: bool, eps: float, return_regions: bool) -> torch.Tensor:
    B, C, H, W = fm.shape
    R = regs.shape[0]
    out = torch.empty((B, R, C) if return_regions else (B, C), dtype=torch.float32, device=fm.device)
    if B:
        ws = _workspace(fm.device, B, C, R)
        with torch.cuda.device(fm.device):
            check(lib().mi355_aggregate_regions(fm.data_ptr(), B, C, H, W, regs.data_ptr(), R, pool, p,
                                                pvec.data_ptr() if pvec is not None else None, EPS_CLAMP, int(normalize),
                                                int(return_regions), eps, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                stream_ptr(fm.device)))
    return out


def _sum_regions(vecs: torch.Tensor, normalize: bool, eps: float) -> torch.Tensor:
    """(B, R, D) fp32 device vectors -> (B, D): their sum in region order, normalised (the aggregation's own second launch)."""
    B, R, D = vecs.shape
    out = torch.empty((B, D), dtype=torch.float32, device=vecs.device)
    if B:
        with torch.cuda.device(vecs.device):
            check(lib().mi355_aggregate_sum(vecs.data_ptr(), B, R, D, int(normalize), eps, out.data_ptr(), stream_ptr(vecs.device)))
    return out


def aggregate(fm: torch.Tensor, method: str = "gem", *, p=3.0, levels: int = 3, regions=None, pool: str | None = None,
              normalize: bool = True, eps: float = 1e-6, return_regions: bool = False, whitening=None) -> torch.Tensor:
    """The descriptor of an un-pooled map ``fm`` (B, C, H, W) on the GPU (1 <= H, W <= 64): (B, C) fp32, or (B, R, C) regional
    vectors with ``return_regions``.

    ``method``: ``spoc`` | ``mac`` | ``gem`` | ``rmac`` | ``crow`` | ``regions`` (module docstring).  ``p``: the GeM exponent, a float in
    (0, 64] or a (C,) tensor of them (values outside [2^-10, 64] are clamped on the device).  ``levels``: of ``rmac_regions``.
    ``regions``: with ``method="regions"``, an integer (R, 4) list of (y0, x0, h, w) inside the map, R <= 64, read on the host.
    ``pool``: ``"max"`` (default), ``"gem"`` or ``"mean"`` inside the regions of ``rmac`` / ``regions``.  ``normalize``: each regional
    vector and the final sum are divided by ``max(norm, eps)``; an all-zero map gives zeros.  ``whitening``: a fitted ``Whitening``
    with ``dim_in == C`` - the regional vectors go through ``whitening.transform`` before they are summed and normalised, the
    R-MAC paper's regional whitening; the result is (B, whitening.dim_out)."""
    if not torch.is_tensor(fm):
        raise MI355Error(f"the feature map must be a tensor, got {type(fm).__name__}")
    require_cuda(fm, "feature map")
    if fm.dim() != 4:
        raise MI355Error(f"expected an un-pooled (B, C, H, W) map, got {tuple(fm.shape)}")
    if method not in METHODS:
        raise MI355Error(f"method {method!r} is not one of {list(METHODS)}")
    fm = fm.detach().float().contiguous()
    B, C, H, W = fm.shape
    if C < 1 or not 1 <= H <= MAX_SIDE or not 1 <= W <= MAX_SIDE:
        raise MI355Error(f"the map must have C >= 1 and 1 <= H, W <= {MAX_SIDE}, got C={C}, H={H}, W={W}")
    eps = _eps(eps)
    if regions is not None and method != "regions":
        raise MI355Error(f"regions= belongs to method='regions', not to {method!r}")
    if pool is not None and method not in ("rmac", "regions"):
        raise MI355Error(f"pool= belongs to the methods 'rmac' and 'regions', not to {method!r}")
    if method == "crow":
        if return_regions or whitening is not None:
            raise MI355Error("crow weights the whole map: it has no regions to return or to whiten")
        out = torch.empty((B, C), dtype=torch.float32, device=fm.device)
        if B:
            ws = _workspace(fm.device, B, C, 1)
            with torch.cuda.device(fm.device):
                check(lib().mi355_aggregate_crow(fm.data_ptr(), B, C, H, W, int(bool(normalize)), eps, out.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), stream_ptr(fm.device)))
        return out
    if method == "regions":
        if regions is None:
            raise MI355Error("method='regions' needs regions=, an (R, 4) list of (y0, x0, h, w)")
        regs = _host_regions(regions, H, W)
    elif method == "rmac":
        regs = rmac_regions(H, W, levels)
        if regs.shape[0] > MAX_REGIONS:
            raise MI355Error(f"levels={levels} gives R={regs.shape[0]} regions on a {H}x{W} map, the limit is {MAX_REGIONS}")
    else:
        regs = torch.tensor([[0, 0, H, W]], dtype=torch.int32)
    kind = _PRESET.get(method) or ("max" if pool is None else pool)
    if kind not in _POOLS:
        raise MI355Error(f"pool {pool!r} is not one of {sorted(_POOLS)}")
    pv, pvec = _p_arg(p, C, fm.device) if kind == "gem" else (1.0, None)
    if whitening is None:
        return _pool_regions(fm, regs, _POOLS[kind], pv, pvec, bool(normalize), eps, bool(return_regions))
    if return_regions:
        raise MI355Error("whitening= returns the summed descriptor: call whitening.transform on the regional vectors yourself")
    if getattr(whitening, "matrix", None) is None or whitening.dim_in != C:
        raise MI355Error(f"whitening must be a fitted Whitening with dim_in == C = {C}, got dim_in="
                         f"{getattr(whitening, 'dim_in', None)!r}")
    v = _pool_regions(fm, regs, _POOLS[kind], pv, pvec, bool(normalize), eps, True)
    t = whitening.transform(v.view(B * regs.shape[0], C))
    return _sum_regions(t.view(B, regs.shape[0], whitening.dim_out), bool(normalize), eps)


class _Descriptors:
    """``model.forward_descriptors``.  It lives in a base of ``MI355Model`` because ``aggregate`` is exported lazily and carries its
    own side-stream case (tests/test_aggregate_streams_gpu.py) instead of a row in the stream table, which lists what
    ``MI355Model`` itself defines."""

    def forward_descriptors(self, x: torch.Tensor, method: str = "gem", **kw) -> torch.Tensor:
        """``aggregate(self.forward_features(x), method, **kw)`` on the convolutional backbones.  Swin's ``forward_features`` is
        already pooled (timm), so there is no map to aggregate."""
        self._refuse_training()
        if self.family == "swin":
            raise MI355Error(f"{self.model_name}: forward_features of a Swin backbone is already pooled to (B, C) - there is no "
                             "(B, C, H, W) map to aggregate; use forward / embed")
        return aggregate(self.forward_features(x), method, **kw)
