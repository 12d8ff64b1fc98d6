"""Torch restatement of the SO(3) log map family (csrc/so3_device.h so3_log_*)
in the dtype of its inputs: fp64 as the tests' yardstick, fp32 to measure what the algorithm
itself loses in that format.  log, relative log, rotation angle, the right Jacobian inverse
J_r^-1, the tangent-space gradients the kernels define, and SO3reparameterize.log_prob through
oracle/lie_ref.so3_log_posterior.  Runs on any device-less machine; a test helper like
tests/vmf_ref.py and tests/losses_ref.py."""
import functools
import math

import torch

from oracle import lie_ref

F64 = torch.float64
SERIES_S = 0.03      # below: asin(s)/s by its series (so3_device.h kLogSeriesS)
SERIES_TH = 0.25     # below: kappa(theta) by its series (so3_device.h kKappaSeriesTh)


# ------------------------------------------------------------------ algebra
def hat(v):
    z = torch.zeros_like(v[..., 0])
    x, y, w = v[..., 0], v[..., 1], v[..., 2]
    return torch.stack([z, -w, y, w, z, -x, -y, x, z], -1).reshape(*v.shape[:-1], 3, 3)


def vee(m):
    return torch.stack((m[..., 2, 1], m[..., 0, 2], m[..., 1, 0]), -1)


def exp(v):
    """Rodrigues with A = sin(th)/th and B = 2 sin^2(th/2)/th^2 (both 1, 1/2 at th = 0), so
    that v = 0 gives I: the yardstick of the round-trip checks, not the library's rodrigues."""
    th = v.norm(dim=-1)
    safe = torch.where(th > 0, th, torch.ones_like(th))
    A = torch.where(th > 1e-4, torch.sin(safe) / safe, 1 - th * th / 6)
    B = torch.where(th > 1e-4, 2 * torch.sin(safe / 2) ** 2 / (safe * safe), 0.5 - th * th / 24)
    K = hat(v)
    eye = torch.eye(3, dtype=v.dtype, device=v.device)
    return eye + A[..., None, None] * K + B[..., None, None] * (K @ K)


# ------------------------------------------------------------------ the log map
def log_polar(R):
    """R (..., 3, 3) -> v (..., 3), theta (...), a (..., 3): a the unit axis (0 where the
    antisymmetric part vanishes and cos >= 0, i.e. at the identity), v = theta a.

    w = vee(R - R^T)/2, s = |w|, c = (tr R - 1)/2, theta = atan2(s, c).  cos >= 0: v =
    (theta/s) w, theta/s = asin(s)/s by its series below SERIES_S.  cos < 0: the axis from
    S = (R + R^T)/2 = c I + (1 - c) a a^T -- the largest a_i^2 = (S_ii - c)/(1 - c) >= 1/3,
    the other two from row i, renormalised, sign so that a.w >= 0; at w = 0 (theta = pi
    exactly) the component of largest magnitude is positive."""
    w = 0.5 * vee(R - R.transpose(-1, -2))
    s = w.norm(dim=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    th = torch.atan2(s, c)
    # cos >= 0
    s2 = s * s
    series = 1 + s2 * (1 / 6 + s2 * (3 / 40 + s2 * (15 / 336)))
    s_safe = torch.where(s > 0, s, torch.ones_like(s))
    k = torch.where(s < SERIES_S, series, th / s_safe)
    v_a = k[..., None] * w
    a_a = torch.where((s > 0)[..., None], w / s_safe[..., None], torch.zeros_like(w))
    # cos < 0
    S = 0.5 * (R + R.transpose(-1, -2))
    omc = 1 - c
    d = (torch.diagonal(S, dim1=-2, dim2=-1) - c[..., None]) / omc[..., None]
    i = torch.argmax(d, dim=-1)
    di = d.gather(-1, i[..., None])[..., 0].clamp(min=1e-30)
    ai = torch.sqrt(di)
    row = S.gather(-2, i[..., None, None].expand(*i.shape, 1, 3))[..., 0, :]
    a = row / (omc * ai)[..., None]
    a = a.scatter(-1, i[..., None], ai[..., None])
    a = a / a.norm(dim=-1, keepdim=True)
    flip = (a * w).sum(-1) < 0
    a_b = torch.where(flip[..., None], -a, a)
    v_b = th[..., None] * a_b
    neg = (c < 0)[..., None]
    return torch.where(neg, v_b, v_a), th, torch.where(neg, a_b, a_a)


def kappa(th):
    """1/th^2 - cot(th/2)/(2 th): 1/12 at 0, 1/pi^2 at pi."""
    t2 = th * th
    series = 1 / 12 + t2 * (1 / 720 + t2 * (1 / 30240 + t2 * (1 / 1209600 + t2 / 47900160)))
    safe = torch.where(th < SERIES_TH, torch.ones_like(th), th)
    h = 0.5 * safe
    direct = 1 / (safe * safe) - torch.cos(h) / (2 * safe * torch.sin(h))
    return torch.where(th < SERIES_TH, series, direct)


def jr_inv(v, th=None):
    """J_r^-1(v) = I + hat(v)/2 + kappa(|v|) hat(v)^2: log(R exp(xi)) = v + J_r^-1 xi + O(xi^2)."""
    if th is None:
        th = v.norm(dim=-1)
    K = hat(v)
    eye = torch.eye(3, dtype=v.dtype, device=v.device)
    return eye + 0.5 * K + kappa(th)[..., None, None] * (K @ K)


def tangent(v, th, gv):
    """u = J_r^-T(v) gv / 2: the gradient of <gv, log(R exp(xi))> in xi is 2 u."""
    return 0.5 * (jr_inv(v, th).transpose(-1, -2) @ gv[..., None])[..., 0]


def log_vjp(R, gv):
    """The tangent-space gradient R hat(u); its component normal to SO(3) is zero."""
    v, th, _ = log_polar(R)
    return R @ hat(tangent(v, th, gv))


class _Log(torch.autograd.Function):
    @staticmethod
    def forward(ctx, R):
        ctx.save_for_backward(R)
        return log_polar(R)[0]

    @staticmethod
    def backward(ctx, gv):
        (R,) = ctx.saved_tensors
        return log_vjp(R, gv)


def log(R):
    """v = log R, differentiable with the tangent-space gradient."""
    return _Log.apply(R)


def rel_log(mu, z):
    """v[s, b] = log(mu[b]^T z[s, b]); mu (B, 3, 3), z (ns, B, 3, 3)."""
    return log(mu.transpose(-1, -2) @ z)


def rel_log_vjp(mu, z, gv):
    """gz = z hat(u), gmu[b] = sum_s mu hat(-Q u), Q = mu^T z."""
    Q = mu.transpose(-1, -2) @ z
    v, th, _ = log_polar(Q)
    u = tangent(v, th, gv)
    gz = z @ hat(u)
    gmu = (mu @ hat(-(Q @ u[..., None])[..., 0])).sum(0)
    return gmu, gz


def angle(A, B):
    return log_polar(A.transpose(-1, -2) @ B)[1]


def angle_vjp(A, B, gth):
    """gB = B hat(gth a / 2), gA = -A hat(gth a / 2); 0 where theta = 0."""
    a = log_polar(A.transpose(-1, -2) @ B)[2]
    H = hat(0.5 * gth[..., None] * a)
    return -(A @ H), B @ H


def log_prob(mu, z, sigma, k=10):
    """log q(z | mu, sigma), (ns, B): the wrapped density of oracle/lie_ref at log(mu^T z)."""
    return lie_ref.so3_log_posterior(rel_log(mu, z), sigma, k)


# ------------------------------------------------------------------ shared inputs
BANDS = ("identity", "tiny", "small", "mid", "large", "near_pi", "half_turn")
BAND_RANGE = {"tiny": (1e-7, 1e-3), "small": (1e-3, 0.1), "mid": (0.1, 3.0),
              "large": (3.0, math.pi - 1e-3), "near_pi": (math.pi - 1e-3, math.pi)}
BAND_N = 257  # one 256-thread block and a tail


def unit_axes(n, gen):
    a = torch.randn(n, 3, generator=gen, dtype=F64)
    a = a / a.norm(dim=-1, keepdim=True)
    # axes along a coordinate, and in a coordinate plane: ties and zeros in the largest-a_i^2 pick
    special = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, 1.0], [0.6, 0.8, 0], [0, -0.6, 0.8],
                            [-0.8, 0, -0.6], [1, 1, 1], [-1, 1, -1]], dtype=F64)
    special = special / special.norm(dim=-1, keepdim=True)
    k = min(n, len(special))
    a[:k] = special[:k]
    return a


@functools.lru_cache(maxsize=None)
def band(name, n=BAND_N):
    """fp64 rotations of one angle band, with their axes and angles: R, a, theta.  `tiny` draws
    theta log-uniformly, the other ranged bands uniformly; `near_pi` excludes pi itself."""
    gen = torch.Generator().manual_seed(7300 + BANDS.index(name))
    a = unit_axes(n, gen)
    if name == "identity":
        th = torch.zeros(n, dtype=F64)
        return torch.eye(3, dtype=F64).expand(n, 3, 3).clone(), a, th
    if name == "half_turn":
        th = torch.full((n,), math.pi, dtype=F64)
        R = 2 * a[:, :, None] * a[:, None, :] - torch.eye(3, dtype=F64)
        return R, a, th
    lo, hi = BAND_RANGE[name]
    u = torch.rand(n, generator=gen, dtype=F64)
    if name == "tiny":
        th = torch.exp(math.log(lo) + u * (math.log(hi) - math.log(lo)))
    elif name == "near_pi":
        th = lo + u * (hi - lo) * (1 - 1e-6)
    else:
        th = lo + u * (hi - lo)
    return exp(a * th[:, None]), a, th


@functools.lru_cache(maxsize=None)
def band_case(name):
    """One band's fp32 input and the fp64 restatement on that same fp32 matrix, computed once
    and shared (left unchanged by its users): R32, v64, th64, a gradient gv and gR64."""
    R32 = band(name)[0].float()
    gen = torch.Generator().manual_seed(7400 + BANDS.index(name))
    gv = torch.randn(R32.shape[0], 3, generator=gen)
    v64, th64, _ = log_polar(R32.double())
    return dict(R=R32, v64=v64, th64=th64, gv=gv, gR64=log_vjp(R32.double(), gv.double()))


def haar(n, gen, dtype=F64):
    q = torch.randn(n, 4, generator=gen, dtype=F64)
    return lie_ref.quat_to_mat(q).to(dtype)


def normwise(y, ref, floor=0.0):
    """|y - ref| over the trailing axes, and the bound's scale |ref| (+ floor)."""
    dims = tuple(range(1, ref.dim()))
    err = (y.double() - ref).flatten(1).norm(dim=-1) if dims else (y.double() - ref).abs()
    scale = ref.flatten(1).norm(dim=-1) if dims else ref.abs()
    return err, scale + floor
