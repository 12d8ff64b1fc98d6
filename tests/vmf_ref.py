"""fp64 torch restatement of the vMF latent on S^3 (csrc/vmf.hip), with the
kernels' noise layout: a sample's row holds 6 T + 3 standard normals, trial t owning g[0..3]
and h[0..1], the last three the tangent direction.  Runs on any device-less machine; the
Bessel values come from scipy.special.ive.  A test helper like tests/losses_ref.py."""
import functools
import math

import numpy as np
import torch
from scipy.special import ive

LOG_AREA_S3 = math.log(2 * math.pi ** 2)
F64 = torch.float64


# ------------------------------------------------------------------ Bessel pieces
def _ive(nu, kappa):
    return torch.from_numpy(np.asarray(ive(nu, kappa.detach().cpu().numpy()), dtype=np.float64))


def _ratio_np(kappa):
    return _ive(2, kappa) / _ive(1, kappa)


class _LogI1Scaled(torch.autograd.Function):
    """ln(I_1(k) e^{-k}); d/dk = I_1'/I_1 - 1 = A + 1/k - 1."""

    @staticmethod
    def forward(ctx, kappa):
        ctx.save_for_backward(kappa)
        return torch.log(_ive(1, kappa))

    @staticmethod
    def backward(ctx, g):
        (kappa,) = ctx.saved_tensors
        return g * (_ratio_np(kappa) + 1 / kappa - 1)


class _Ratio(torch.autograd.Function):
    """A = I_2 / I_1; A' = 1 - A^2 - 3 A / k."""

    @staticmethod
    def forward(ctx, kappa):
        ctx.save_for_backward(kappa)
        return _ratio_np(kappa)

    @staticmethod
    def backward(ctx, g):
        (kappa,) = ctx.saved_tensors
        return g * ratio_prime(kappa)


def ratio(kappa):
    """A(kappa) = I_2 / I_1 = E[mu.z]."""
    return _Ratio.apply(kappa)


def ratio_prime(kappa):
    """A'(kappa) = Var[mu.z]."""
    A = _ratio_np(kappa)
    return 1 - A * A - 3 * A / kappa


def log_norm_shifted(kappa):
    """ln C + kappa, C = kappa / ((2 pi)^2 I_1(kappa))."""
    return torch.log(kappa) - 2 * math.log(2 * math.pi) - _LogI1Scaled.apply(kappa)


def kl(kappa):
    """KL(vMF(., kappa) || U(S^3)) = kappa A + ln C + ln(2 pi^2), (B,)."""
    return -kappa * (1 - ratio(kappa)) + log_norm_shifted(kappa) + LOG_AREA_S3


def dkl_dkappa(kappa):
    return kappa * ratio_prime(kappa)


# ------------------------------------------------------------------ sampler
def trials_of(noise):
    W = noise.shape[-1]
    assert W >= 9 and (W - 3) % 6 == 0, W
    return (W - 3) // 6


def constants(kappa):
    c = torch.sqrt(4 * kappa ** 2 + 9)
    b = 3 / (2 * kappa + c)
    a = (3 + 2 * kappa + c) / 4
    d = 4 * a * b / (1 + b) - 3 * math.log(3.0)
    return a, b, c, d


def proposal(g):
    """g (..., 4) normals -> eps = (1 + x)/2 and 1 - eps, x = g0/|g|, without subtraction."""
    g0 = g[..., 0]
    s = (g[..., 1:] ** 2).sum(-1)
    n = torch.sqrt(s + g0 * g0)
    small = s / (n * (n + g0.abs()))
    big = 1 + g0.abs() / n
    pos = g0 > 0
    return torch.where(pos, big, small) / 2, torch.where(pos, small, big) / 2


def margins(kappa, noise):
    """lhs - rhs of the acceptance test for every trial, (ns, B, T), with eps and 1 - eps."""
    T = trials_of(noise)
    tr = noise[..., :6 * T].reshape(*noise.shape[:-1], T, 6)
    a, b, _, d = (t[None, :, None] for t in constants(kappa))
    e, eb = proposal(tr[..., :4])
    t = 2 * a * b / (eb + b * e)
    lhs = 3 * torch.log(t) - t + d
    rhs = -(tr[..., 4] ** 2 + tr[..., 5] ** 2) / 2
    return lhs - rhs, e, eb


def first_accepted(margin):
    """Index of the first trial with margin >= 0, or T when there is none."""
    T = margin.shape[-1]
    idx = torch.arange(T).expand_as(margin)
    return torch.where(margin >= 0, idx, torch.full_like(idx, T)).min(-1).values


def reflect(mu, x):
    """The orthogonal map taking e1 to mu, applied to x (ns, B, 4): two branches."""
    sgn = torch.where(mu[..., :1] <= 0, 1.0, -1.0).to(mu.dtype)
    e1 = torch.zeros_like(mu)
    e1[..., 0] = 1
    u = e1 - sgn * mu
    y = x - 2 * u * (u * x).sum(-1, keepdim=True) / (u * u).sum(-1, keepdim=True)
    return sgn * y


def sample(mu, kappa, noise, accepted=None):
    """mu (B, 4) or (ns, B, 4), kappa (B) or (ns, B), noise (ns, B, 6T+3), all fp64 ->
    z (ns, B, 4), accepted (ns, B) int64, margin (ns, B, T).  `accepted` given: that trial is
    used (frozen indices, for gradients).  The value T means the last proposal."""
    T = trials_of(noise)
    kap_b = kappa if kappa.dim() == 1 else kappa[0]
    margin, e, eb = margins(kap_b.detach(), noise)
    if accepted is None:
        accepted = first_accepted(margin)
    pick = accepted.clamp(max=T - 1)[..., None]
    e, eb = e.gather(-1, pick)[..., 0], eb.gather(-1, pick)[..., 0]
    b = constants(kappa)[1]
    D = eb + b * e
    w = (eb - b * e) / D
    r = 2 * torch.sqrt(b * e * eb) / D
    tn = noise[..., 6 * T:]
    v = tn / tn.norm(dim=-1, keepdim=True)
    x = torch.cat([w[..., None], r[..., None] * v], -1)
    return reflect(mu, x), accepted, margin


def log_prob(mu, kappa, z):
    """(ln C + kappa) - kappa |z - mu|^2 / 2, (ns, B)."""
    return log_norm_shifted(kappa) - kappa * ((z - mu) ** 2).sum(-1) / 2


def _per_sample(mu, kappa, ns):
    """mu and kappa repeated per sample, as leaves: their gradients are the per-sample terms."""
    mu_s = mu.detach()[None].expand(ns, -1, -1).clone().requires_grad_(True)
    kap_s = kappa.detach()[None].expand(ns, -1).clone().requires_grad_(True)
    return mu_s, kap_s


def sample_grads(mu, kappa, noise, accepted, gz):
    """fp64 autograd of `sample` on frozen indices: gmu (B, 4), gkappa (B), and the per-sample
    terms (ns, B, 4) and (ns, B) whose sums over s they are."""
    mu_s, kap_s = _per_sample(mu, kappa, noise.shape[0])
    z, _, _ = sample(mu_s, kap_s, noise, accepted)
    z.backward(gz)
    return mu_s.grad.sum(0), kap_s.grad.sum(0), mu_s.grad, kap_s.grad


def log_prob_grads(mu, kappa, z, gout):
    """fp64 autograd of `log_prob`: gmu (B, 4), gkappa (B), gz (ns, B, 4) and the per-sample
    terms of the first two."""
    mu_s, kap_s = _per_sample(mu, kappa, z.shape[0])
    zz = z.detach().clone().requires_grad_(True)
    out = log_norm_shifted(kap_s) - kap_s * ((zz - mu_s) ** 2).sum(-1) / 2
    out.backward(gout)
    return mu_s.grad.sum(0), kap_s.grad.sum(0), zz.grad, mu_s.grad, kap_s.grad


# ------------------------------------------------------------------ shared inputs
KAPPAS = (1.0, 1.5, 10.0, 100.0, 1e3, 1e5)


def haar_mu(B, gen):
    """Unit 4-vectors in fp32 (as the module normalises them): Haar-uniform, with the rows
    +e1, -e1, one with mu[0] = 0 and one within 1e-4 of e1 placed first where B allows."""
    mu = torch.randn(B, 4, generator=gen, dtype=F64)
    special = torch.tensor([[1.0, 0, 0, 0], [-1.0, 0, 0, 0], [0, 0.6, 0, 0.8],
                            [1.0, 6e-5, -5e-5, 3e-5]], dtype=F64)
    k = min(B - 1, 4) if B > 1 else 0
    mu[:k] = special[:k]
    mu = mu.float()
    return mu / mu.norm(dim=-1, keepdim=True)


def cycle_kappa(B):
    return torch.tensor([KAPPAS[i % len(KAPPAS)] for i in range(B)], dtype=torch.float32)


PARITY_SHAPES = ((1, 1), (2, 3), (3, 67), (4, 2048))
MARGIN_EXCLUDE = 1e-4   # a sample with an acceptance margin this small is not compared
MAX_EXCLUDED = 1e-3     # fraction of the samples that may be left out for that reason


@functools.lru_cache(maxsize=None)
def parity_case(ns, B, trials=16):
    """Inputs (fp32) and the fp64 restatement's results for one sampler case, computed once
    and shared: mu, kappa, noise, z, accepted, margin, and `close`, the samples where some
    trial up to and including the accepted one has |margin| < MARGIN_EXCLUDE (an fp32
    evaluation may decide such a trial the other way)."""
    gen = torch.Generator().manual_seed(4100 + 17 * ns + B + 1000 * trials)
    mu, kappa = haar_mu(B, gen), cycle_kappa(B)
    noise = torch.randn(ns, B, 6 * trials + 3, generator=gen)
    z, acc, margin = sample(mu.double(), kappa.double(), noise.double())
    upto = torch.arange(trials) <= acc.clamp(max=trials - 1)[..., None]
    close = ((margin.abs() < MARGIN_EXCLUDE) & upto).any(-1)
    return dict(mu=mu, kappa=kappa, noise=noise, z=z, accepted=acc, margin=margin, close=close)


def normwise(y, ref):
    """|y - ref| / |ref| over the last axis."""
    return (y.double() - ref).norm(dim=-1) / ref.norm(dim=-1)
