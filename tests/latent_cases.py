"""Seeded cases and the fp64 yardstick for the SO(3) normal latent kernels of
csrc/pointwise.hip (lv_so3_log_posterior_*, lv_so3_sample_*, lv_n0_sample_*, lv_softplus_*).

The yardstick is oracle/lie_ref.py under torch autograd, in float64; the "reference's fp32
error" is the same oracle in float32 on the same (fp32-representable) inputs against that.

A density batch is laid out in cells: a radius band for |v| crossed with a class of sigma.
sigma belongs to b, so b fixes the cell (cell = b mod 36: class = b mod 4, band = (b / 4) mod 9)
and every s of a b shares it; ns = 3, B = 240 gives 18 or 21 samples (6 or 7 b) per cell.
A band is a distance to the nearest multiple of pi; the jitter (up to +5%) scales that distance,
so a band stays on its side of the two clamps of the volume term,
max(thk^2, 1e-3) / max(2 - 2 cos thk, 1e-3) (oracle/lie_ref.py so3_log_posterior).

The density is per sample (lp[s, b] depends on v[s, b] and sigma[b] alone), so the yardstick is
computed once per k for the 720 base samples -- value, d lp / d v and d lp / d sigma -- and any
arrangement (ns, B, gout) of those samples is composed from it in fp64 (`arrange`, `compose`):
gv[s, b] = gout[s, b] * dv, gsigma[b] = sum_s gout[s, b] * dsigma.  A tiled or ragged batch so
keeps each sample's cell and the cell's reference error, at no cost in fp64 evaluations.
"""
import functools
import math

import numpy as np
import torch

from oracle import lie_ref

F32, F64 = torch.float32, torch.float64
PI = math.pi

# (centre, signed distance): |v| = centre + distance * (1 + 0.05 u), u in [0, 1)
BANDS = (
    ("0.004", 0.0, 0.004),          # both clamps active at t = 0
    ("0.02", 0.0, 0.02),            # both clamps active at t = 0
    ("0.06", 0.0, 0.06),            # just above the clamps: fp32 cancellation in 2 - 2cos
    ("0.7", 0.0, 0.7),
    ("pi-1e-3", PI, -1e-3),
    ("pi+0.2", PI, 0.2),
    ("2pi-0.01", 2 * PI, -0.01),    # clamps active at t = -1
    ("2pi+0.012", 2 * PI, 0.012),   # clamps active at t = -1
    ("9.0", 0.0, 9.0),
)
CLASSES = ("narrow", "unit", "broad", "aniso")
NBAND, NCLASS = len(BANDS), len(CLASSES)
NCELL = NBAND * NCLASS
NS0, B0 = 3, 240
KS = (0, 1, 2, 10, 31, 32, 33, 64)
SEED = 20240

# the project's bounds for this op (tests/test_gpu_parity.py test_log_posterior_wide_range)
VAL_RTOL, VAL_ATOL, GRAD_TOL = 1e-5, 1e-4, 1e-4
CLAMP_EDGE = (0.8e-3, 1.25e-3)


def sigma_range(cls, k):
    w = PI * max(k, 1)
    return {"narrow": (0.03, 0.3), "unit": (0.3, 3.0), "broad": (0.5 * w, 1.5 * w),
            "aniso": (0.03, w)}[cls]


def cell_of_b(b):
    """Cell index (band * NCLASS + class) of base column b."""
    b = np.asarray(b)
    return ((b // NCLASS) % NBAND) * NCLASS + b % NCLASS


def cell_name(c):
    return f"{BANDS[c // NCLASS][0]} x {CLASSES[c % NCLASS]}"


def radii(band, n, gen):
    _, centre, dist = BANDS[band]
    return centre + dist * (1 + 0.05 * torch.rand(n, generator=gen, dtype=F64))


def unit_vectors(n, gen):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, dtype=F64), dim=-1)


def per_sample(v, sigma, k, dtype):
    """The oracle and its autograd on N independent samples (each with its own sigma row):
    lp (N), d lp / d v (N, 3), d lp / d sigma (N, 3), as float64 arrays."""
    v = v.to(dtype).reshape(1, -1, 3).clone().requires_grad_(True)
    s = sigma.to(dtype).clone().requires_grad_(True)
    lp = lie_ref.so3_log_posterior(v, s, k)
    lp.sum().backward()
    return tuple(t.detach().double().numpy() for t in (lp[0], v.grad[0], s.grad))


def rel_rows(y, ref):
    """||y - ref|| / ||ref|| per row, in fp64."""
    y = np.asarray(y, np.float64).reshape(len(ref), -1)
    r = np.asarray(ref, np.float64).reshape(len(ref), -1)
    return np.linalg.norm(y - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300)


class Case:
    """The 720 base samples at one k: inputs (fp32 tensors), the fp64 yardstick and the fp32
    oracle per sample, flattened s-major (sample s * B0 + b)."""

    def __init__(self, k, seed=SEED):
        self.k = k
        gen = torch.Generator().manual_seed(seed + 1000 * k)
        cell = cell_of_b(np.arange(B0))
        sigma = torch.empty(B0, 3, dtype=F64)
        v = torch.empty(NS0, B0, 3, dtype=F64)
        for b in range(B0):
            lo, hi = sigma_range(CLASSES[cell[b] % NCLASS], k)
            sigma[b] = lo * (hi / lo) ** torch.rand(3, generator=gen, dtype=F64)
            v[:, b] = radii(cell[b] // NCLASS, NS0, gen)[:, None] * unit_vectors(NS0, gen)
        self.v, self.sigma = v.to(F32), sigma.to(F32)
        self.gout = torch.randn(NS0, B0, generator=gen, dtype=F64).to(F32)
        self.cell_b = cell                       # (B0,)
        self.cell = np.tile(cell, NS0)           # (720,)
        sig_rows = self.sigma.repeat(NS0, 1)     # sample s * B0 + b -> sigma[b]
        self.lp64, self.dv64, self.ds64 = per_sample(self.v, sig_rows, k, F64)
        self.lp32, self.dv32, self.ds32 = per_sample(self.v, sig_rows, k, F32)

    def theta64(self):
        return self.v.double().norm(dim=-1).reshape(-1).numpy()

    def cell_max(self, err, cell):
        """Worst err per cell, as an array over the NCELL cells (0 where a cell is absent)."""
        out = np.zeros(NCELL)
        np.maximum.at(out, cell, err)
        return out


@functools.lru_cache(maxsize=None)
def case(k, seed=SEED):
    return Case(k, seed)


def arrange(ns, B, stride=1):
    """Base sample of element (s, b) of an (ns, B) batch: s mod 3 and (stride * b) mod 240.
    Returns (base column per b (B,), base sample per element (ns, B))."""
    col = (stride * np.arange(B)) % B0
    return col, (np.arange(ns)[:, None] % NS0) * B0 + col[None, :]


def inputs(c, ns, B, stride=1):
    """(v (ns, B, 3), sigma (B, 3), gout (ns, B)) fp32: the base batch gathered by `arrange`
    (gout is gathered too, so a tiled gsigma is the base one times its repeat count and sums
    without cancellation the base batch does not have)."""
    col, samp = arrange(ns, B, stride)
    samp = torch.from_numpy(samp)
    return (c.v.reshape(-1, 3)[samp], c.sigma[torch.from_numpy(col)], c.gout.reshape(-1)[samp])


def compose(c, ns, B, stride=1, dtype="64"):
    """lp (ns, B), gv (ns, B, 3), gsigma (B, 3) of `inputs(c, ns, B, stride)` from the
    per-sample yardstick (dtype "64") or the fp32 oracle ("32"); the composition is in fp64."""
    _, samp = arrange(ns, B, stride)
    lp, dv, ds = (getattr(c, n + dtype) for n in ("lp", "dv", "ds"))
    g = c.gout.double().numpy().reshape(-1)[samp]
    return lp[samp], g[..., None] * dv[samp], (g[..., None] * ds[samp]).sum(0)


def grade(c, ns, B, lp, gv, gs, stride=1):
    """Worst ratio of the error against fp64 to the bound, for the values, gv and gsigma of one
    run: a sample (a b, for gsigma) is within bound when its error is within the project's
    tolerance or within 2x the worst fp32-oracle error of its own cell.  Returns
    {"lp": (ratio, where), "gv": ..., "gsigma": ...}; a ratio <= 1 passes; non-finite -> inf."""
    col, samp = arrange(ns, B, stride)
    cell_s, cell_b = c.cell[samp].reshape(-1), c.cell_b[col]
    lp64, gv64, gs64 = compose(c, ns, B, stride, "64")
    lp32, gv32, gs32 = compose(c, ns, B, stride, "32")
    out = {}

    def ratio(err, tol, eref, cell, what):
        bound = np.maximum(tol, 2 * c.cell_max(eref, cell)[cell])
        r = np.where(np.isfinite(err), err / bound, np.inf)
        i = int(np.argmax(r))
        out[what] = (float(r[i]), f"{what}[{i}] cell {cell_name(cell[i])}: err {err[i]:.3e} "
                                  f"bound {bound[i]:.3e}")

    lp, lp64f, lp32f = (np.asarray(a, np.float64).reshape(-1) for a in (lp, lp64, lp32))
    ratio(np.abs(lp - lp64f), VAL_ATOL + VAL_RTOL * np.abs(lp64f), np.abs(lp32f - lp64f),
          cell_s, "lp")
    gv64f = gv64.reshape(-1, 3)
    ratio(rel_rows(np.asarray(gv).reshape(-1, 3), gv64f), GRAD_TOL,
          rel_rows(gv32.reshape(-1, 3), gv64f), cell_s, "gv")
    ratio(rel_rows(gs, gs64), GRAD_TOL, rel_rows(gs32, gs64), cell_b, "gsigma")
    return out


# ------------------------------------------------------------------ companions
def softplus_points():
    """The edge inputs of the softplus kernels: the threshold 20 with its fp32 neighbours, the
    exp overflow at ~88.7, deep tails."""
    t = np.float32(20.0)
    return np.array([-100.0, -20.0, 0.0, np.nextafter(t, np.float32(-np.inf)), t,
                     np.nextafter(t, np.float32(np.inf)), 20.5, 88.0, 89.0, 1e4], np.float32)


def softplus_bulk(n, seed=SEED):
    """Uniform on [-30, 30): both sides of the threshold."""
    gen = torch.Generator().manual_seed(seed + 7)
    return ((torch.rand(n, generator=gen, dtype=F64) - 0.5) * 60).to(F32)


def band_vectors(ns, B, seed=SEED):
    """v (ns, B, 3) fp32 with |v| from the radius bands, band = b mod 9."""
    gen = torch.Generator().manual_seed(seed + 11)
    v = torch.empty(ns, B, 3, dtype=F64)
    for b in range(B):
        v[:, b] = radii(b % NBAND, ns, gen)[:, None] * unit_vectors(ns, gen)
    return v.to(F32), np.arange(B) % NBAND


def large_lse_case(B=64, seed=SEED):
    """(v (1, B, 3), sigma (B, 3)) fp32 with |v| in the band pi - 1e-3 and sigma log-uniform in
    [0.02, 0.03]: log q ~ -|v|^2 / (2 sigma^2) is about -1e4, where an fp32 ulp is 1e-3, yet the
    gradients are well conditioned (the fp32 oracle keeps them to 1e-5).  The smallest case
    that told a backward forming its weights as exp(l_t - lse), lse rounded to fp32, from
    one forming exp(l_t - m) / sum."""
    gen = torch.Generator().manual_seed(seed + 13)
    sigma = 0.02 * 1.5 ** torch.rand(B, 3, generator=gen, dtype=F64)
    band = [b[0] for b in BANDS].index("pi-1e-3")
    v = radii(band, B, gen)[:, None] * unit_vectors(B, gen)
    return v.to(F32)[None], sigma.to(F32)


def two_mode_case(B=64, seed=SEED):
    """(v (1, B, 3), sigma (B, 3)) fp32 with |v| in the band pi - 1e-3 and sigma log-uniform in
    [0.05, 0.3]: the wrapped terms t = 0 and t = -1 lie at +-pi with comparable weights and
    slopes -+|v| q, q = sum_j (u_j / sigma_j)^2 in the hundreds, so the gradient is a difference
    of weights that follow l_0 - l_-1, a difference of two terms of size 1e2..1e3.  An fp32
    evaluation of the terms (the fp32 oracle included) is off by up to a few 1e-4 here; one that
    takes the Gaussian part of the weights in fp64 holds 1e-4."""
    gen = torch.Generator().manual_seed(seed + 17)
    sigma = 0.05 * 6.0 ** torch.rand(B, 3, generator=gen, dtype=F64)
    band = [b[0] for b in BANDS].index("pi-1e-3")
    v = radii(band, B, gen)[:, None] * unit_vectors(B, gen)
    return v.to(F32)[None], sigma.to(F32)
