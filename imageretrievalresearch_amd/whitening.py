"""PCA whitening and dimension reduction of embeddings (Radenovic, Tolias and Chum, TPAMI 2018: "descriptors are
L2-normalised, whitened, re-normalised"), the step that comes before query expansion / database-side augmentation.

* ``embedding_moments`` ... float64 first and second raw moments of rows on the GPU (``mi355_embedding_moments``)
* ``Whitening.fit`` ....... moments on the GPU, then ``from_moments``
* ``Whitening.from_moments`` ... mean, covariance, eigen-decomposition and the projection, all host float64 (no GPU)
* ``Whitening.transform`` ..... normalise -> project -> bias -> normalise in one HIP launch (``mi355_whiten_rows``)

Order of the post-processing steps: whiten first, then ``qe=`` / ``Gallery.augmented`` on the whitened rows.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import rank as _rank
from ._lib import MI355Error, check, lib, require_cuda, stream_ptr

_EPS = _rank._EPS


class Moments(NamedTuple):
    n: int                    # rows summed
    sum: torch.Tensor         # (D,) float64, sum_r x[r]
    outer: torch.Tensor       # (D, D) float64, sum_r x[r] x[r]^T, exactly symmetric


def _strided_rows(t: torch.Tensor, name: str) -> torch.Tensor:
    """An fp32 (R, D) device tensor whose rows a kernel can read: rows with unit element stride are used where they lie (row
    stride >= D), anything else is made contiguous."""
    if not torch.is_tensor(t):
        raise MI355Error(f"{name} must be a tensor or a Gallery, got {type(t).__name__}")
    require_cuda(t, name)
    if t.dim() != 2:
        raise MI355Error(f"{name} must be (rows, dim), got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        if not t.dtype.is_floating_point:
            raise MI355Error(f"{name} must hold floats, got {t.dtype}")
        t = t.float()
    R, D = t.shape
    if R > 1 and D >= 1 and (t.stride(1) == 1 or D == 1) and t.stride(0) >= D:
        return t
    return t.contiguous()


def _source(rows, name: str) -> "_rank._Rows":
    """The rows a moments call reads, where they lie: the resident rows of a Gallery (or of a shard), or a tensor's."""
    if isinstance(rows, _rank.Gallery):
        rows = rows._resident()
    if isinstance(rows, _rank._Rows):
        require_cuda(rows.buf, name)
        return rows
    t = _strided_rows(rows, name)
    return _rank._Rows(t, t.shape[0], t.shape[1], False)


def _moments_into(src, normalize, eps, accumulate, s, o):
    R, dim = src.shape
    if dim < 1:
        raise MI355Error(f"embedding_moments needs dim >= 1, got {dim}")
    ws = _rank._ws.get(src.device, max(int(lib().mi355_moments_workspace_bytes(R, dim)), 1))
    with torch.cuda.device(src.device):
        check(lib().mi355_embedding_moments(src.buf.data_ptr() if R else None, _rank._DTYPES[src.dtype], R, src.ld, dim,
                                            int(bool(normalize)), float(eps), int(bool(accumulate)), s.data_ptr(), o.data_ptr(),
                                            ws.data_ptr(), ws.numel(), stream_ptr(src.device)))


def embedding_moments(rows, *, normalize: bool = False, eps: float = _EPS, out: Moments | None = None) -> Moments:
    """``Moments(n, sum, outer)`` of ``rows``: a (R, D) fp32 device tensor (rows may be strided), or a ``Gallery`` (its resident
    normalised rows, fp32 or fp16).  ``normalize=True`` (fp32 tensors) takes ``l2_normalize_rows(rows, eps)`` - same bits -
    without writing it.  Elements are widened to float64, products and sums are float64 (f64 MFMA); the result is the same
    bits on every run.  ``out=`` (a ``Moments`` of the same D on the same device) is added to: a streaming fit."""
    src = _source(rows, "rows")
    (R, dim), device = src.shape, src.device
    if normalize and src.dtype != torch.float32:
        raise MI355Error("normalize=True needs fp32 rows (a Gallery's rows are normalised already)")
    if out is None:
        s = torch.empty((dim,), dtype=torch.float64, device=device)
        o = torch.empty((dim, dim), dtype=torch.float64, device=device)
        n0 = 0
    else:
        n0, s, o = out
        for t, shape, nm in ((s, (dim,), "sum"), (o, (dim, dim), "outer")):
            if (not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != device
                    or not t.is_contiguous()):
                raise MI355Error(f"out.{nm} must be a contiguous float64 {shape} tensor on {device}")
    _moments_into(src, normalize, eps, out is not None, s, o)
    return Moments(int(n0) + R, s, o)


def _host64(t, name: str) -> torch.Tensor:
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not torch.is_tensor(t):
        raise MI355Error(f"{name} must be a float64 tensor or array, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise MI355Error(f"{name} must be float64, got {t.dtype}")
    return t.detach().cpu()


class Whitening:
    """A fitted PCA whitening: ``y = normalise(matrix @ normalise(x) + bias)`` with ``matrix = diag(scale) V^T`` of the
    covariance's leading ``dim_out`` eigenvectors and ``bias = -matrix @ mean``.

    Attributes: ``dim_in``, ``dim_out``, ``mean`` (D,) f32, ``matrix`` (d, D) f32, ``bias`` (d,) f32, ``eigenvalues`` (D,) f64
    descending, ``explained_variance_ratio`` (d,) f64, ``power``, ``ridge``, ``normalize_input``, ``num_rows``."""

    eps = _EPS

    def __init__(self):
        self.dim_in = self.dim_out = self.num_rows = 0
        self.mean = self.matrix = self.bias = self.eigenvalues = self.explained_variance_ratio = None
        self.power, self.ridge, self.normalize_input = 0.5, 1e-5, True

    # ---- fit
    @classmethod
    def fit(cls, rows, dim_out: int | None = None, *, power: float = 0.5, ridge: float = 1e-5, normalize_input: bool = True,
            block: int = 65536) -> "Whitening":
        """Fit on a (R, D) fp32 device tensor (``block`` rows per moments call, accumulated; ``normalize_input`` normalises
        each row first, without a copy) or on a ``Gallery`` (its resident normalised rows, fp32 or fp16, as they are;
        ``normalize_input`` then only records that queries must be normalised)."""
        if isinstance(rows, _rank.Gallery):
            m = embedding_moments(rows)
        else:
            t = _strided_rows(rows, "rows")
            block = max(int(block), 1)
            m = None
            for r0 in range(0, max(t.shape[0], 1), block):
                part = embedding_moments(t[r0: r0 + block], normalize=normalize_input, eps=cls.eps, out=m)
                m = part
        return cls.from_moments(m.n, m.sum, m.outer, dim_out, power=power, ridge=ridge, normalize_input=normalize_input,
                                device=m.sum.device)

    @classmethod
    def from_moments(cls, n, sum, outer, dim_out: int | None = None, *, power: float = 0.5, ridge: float = 1e-5,
                     normalize_input: bool = True, device=None) -> "Whitening":
        """The transform of ``n`` rows with moments ``sum`` (D,) / ``outer`` (D, D) (float64 tensors or arrays, any device):
        mu = sum / n, C = outer / n - mu mu^T symmetrised, ``torch.linalg.eigh`` on the CPU in float64, eigenvalues clamped at 0
        and sorted descending, each eigenvector signed so that its component of largest magnitude (lowest index on a tie) is
        positive, scale_j = (lambda_j + ridge * lambda_0) ** -power, matrix = diag(scale[:d]) V[:, :d]^T, bias = -matrix mu;
        both rounded once to fp32.  power 0.5 whitens, 0 is the plain PCA rotation / truncation.  Needs no GPU."""
        if not _rank._is_int(n):
            raise MI355Error(f"n must be an integer row count, got {n!r}")
        n = int(n)
        if n < 2:
            raise MI355Error(f"a whitening fit needs at least 2 rows, got n={n}")
        s, o = _host64(sum, "sum"), _host64(outer, "outer")
        if s.dim() != 1 or s.shape[0] < 1 or o.dim() != 2 or tuple(o.shape) != (s.shape[0], s.shape[0]):
            raise MI355Error(f"moments must be sum (D,) and outer (D, D), got {tuple(s.shape)} and {tuple(o.shape)}")
        D = int(s.shape[0])
        d = D if dim_out is None else dim_out
        if not _rank._is_int(d) or not 1 <= int(d) <= D:
            raise MI355Error(f"dim_out must be an integer in [1, {D}], got {dim_out!r}")
        d = int(d)
        try:
            power, ridge = float(power), float(ridge)
        except (TypeError, ValueError):
            raise MI355Error(f"power and ridge must be floats >= 0, got {power!r} and {ridge!r}") from None
        if not np.isfinite(power) or power < 0:
            raise MI355Error(f"power must be a finite float >= 0, got {power!r}")
        if not np.isfinite(ridge) or ridge < 0:
            raise MI355Error(f"ridge must be a finite float >= 0, got {ridge!r}")
        if not bool(torch.isfinite(s).all()) or not bool(torch.isfinite(o).all()):
            raise MI355Error("the moments hold NaN or Inf (a non-finite embedding row went into the fit)")
        mu = s / n
        C = o / n - torch.outer(mu, mu)
        C = (C + C.t()) * 0.5
        lam, V = torch.linalg.eigh(C)
        lam = lam.clamp_min(0.0).flip(0).contiguous()
        V = V.flip(1).contiguous()
        cols = torch.arange(D)
        top = V.abs().argmax(dim=0)                               # first index of the largest magnitude
        sign = torch.where(V[top, cols] < 0, -1.0, 1.0).to(torch.float64)
        V = V * sign[None, :]
        base = lam[:d] + ridge * lam[0]
        if power > 0 and bool((base <= 0).any()):
            raise MI355Error("a kept eigenvalue is zero and ridge does not lift it: whitening (power > 0) would divide by zero; "
                             "lower dim_out or set ridge > 0")
        scale = torch.ones(d, dtype=torch.float64) if power == 0 else base ** (-power)
        matrix = scale[:, None] * V[:, :d].t()
        bias = -(matrix @ mu)
        w = cls()
        w.dim_in, w.dim_out, w.num_rows = D, d, n
        w.power, w.ridge, w.normalize_input = power, ridge, bool(normalize_input)
        w.mean = mu.to(torch.float32)
        w.matrix = matrix.to(torch.float32).contiguous()
        w.bias = bias.to(torch.float32).contiguous()
        w.eigenvalues = lam
        total = float(lam.sum())
        w.explained_variance_ratio = lam[:d] / total if total > 0 else torch.zeros(d, dtype=torch.float64)
        return w.to(device) if device is not None else w

    # ---- state
    _TENSORS = ("mean", "matrix", "bias", "eigenvalues", "explained_variance_ratio")
    _SCALARS = ("dim_in", "dim_out", "num_rows", "power", "ridge", "normalize_input")

    def state_dict(self) -> dict:
        sd = {k: getattr(self, k).detach().cpu().clone() for k in self._TENSORS}
        sd.update({k: getattr(self, k) for k in self._SCALARS})
        return sd

    def load_state_dict(self, sd: dict) -> "Whitening":
        missing = [k for k in self._TENSORS + self._SCALARS if k not in sd]
        if missing:
            raise MI355Error(f"whitening state_dict lacks {missing}")
        D, d = int(sd["dim_in"]), int(sd["dim_out"])
        want = {"mean": ((D,), torch.float32), "matrix": ((d, D), torch.float32), "bias": ((d,), torch.float32),
                "eigenvalues": ((D,), torch.float64), "explained_variance_ratio": ((d,), torch.float64)}
        device = self.matrix.device if self.matrix is not None else torch.device("cpu")
        for k, (shape, dt) in want.items():
            t = sd[k]
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt:
                raise MI355Error(f"whitening state_dict: {k} must be a {dt} tensor of shape {shape}")
        for k in self._TENSORS:
            setattr(self, k, sd[k].detach().clone().contiguous())
        self.dim_in, self.dim_out, self.num_rows = D, d, int(sd["num_rows"])
        self.power, self.ridge, self.normalize_input = float(sd["power"]), float(sd["ridge"]), bool(sd["normalize_input"])
        return self.to(device)

    def to(self, device) -> "Whitening":
        """The same transform with ``mean`` / ``matrix`` / ``bias`` on ``device`` (in place; the float64 spectra stay on the host)."""
        for k in ("mean", "matrix", "bias"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    # ---- transform
    def _apply(self, src, normalize_input, out, normalize_output):
        """One mi355_whiten_rows launch of the rows ``src`` (``rank._Rows``, fp32 or fp16) into the rows of ``out`` ((R, >= dim_out)
        fp32 or fp16 gallery rows)."""
        if self.matrix is None:
            raise MI355Error("this Whitening is not fitted")
        if self.matrix.device != out.device:
            raise MI355Error(f"the whitening lives on {self.matrix.device} but the rows on {out.device}: call .to(device)")
        R = src.rows
        if R == 0:
            return out
        out_dt = _rank._DTYPES[out.dtype]
        ws = _rank._ws.get(out.device, max(int(lib().mi355_whiten_workspace_bytes(R, self.dim_in, self.dim_out, out_dt)), 1))
        with torch.cuda.device(out.device):
            check(lib().mi355_whiten_rows(src.buf.data_ptr(), _rank._DTYPES[src.dtype], R, src.ld, self.dim_in,
                                          int(bool(normalize_input)), float(self.eps), self.matrix.data_ptr(), self.bias.data_ptr(),
                                          self.dim_out, int(bool(normalize_output)), out.data_ptr(), out_dt, _rank._row_stride(out),
                                          ws.data_ptr(), ws.numel(), stream_ptr(out.device)))
        return out

    def transform(self, x: torch.Tensor, *, normalize_output: bool = True, out: torch.Tensor | None = None) -> torch.Tensor:
        """(R, dim_in) fp32 device rows -> (R, dim_out) fp32: ``l2_normalize_rows(matrix @ x' + bias)`` with x' =
        ``l2_normalize_rows(x)`` when the fit has ``normalize_input`` (both bit for bit the library's normalisation), fp32
        products and accumulation in a fixed order: a row's result does not depend on the batch it is in.  One HIP launch."""
        t = _strided_rows(x, "x")
        if t.shape[1] != self.dim_in:
            raise MI355Error(f"x must be (R, {self.dim_in}), got {tuple(t.shape)}")
        R = int(t.shape[0])
        if out is None:
            out = torch.empty((R, self.dim_out), dtype=torch.float32, device=t.device)
        elif (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (R, self.dim_out)
              or out.device != t.device or not out.is_contiguous()):
            raise MI355Error(f"out must be a contiguous fp32 ({R}, {self.dim_out}) tensor on {t.device}")
        return self._apply(_rank._Rows(t, R, self.dim_in, False), self.normalize_input, out, normalize_output)
