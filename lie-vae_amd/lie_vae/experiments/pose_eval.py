"""Pose evaluation: did the encoder learn the pose?  (Extension; the reference has no such
script.)

The latent of an action-decoder VAE is identified only up to a fixed rotation on each side:
D(z·h)·F = D(z)·(D(h)·F) and h is absorbed by the learned ``item_rep``, and the data's own
frame is arbitrary on the left.  The posterior mean rotations are therefore aligned to the
ground-truth poses first -- ``lie_tools.align_rotations``, min over (A, B) of
Σ‖z_i − A·g_i·B‖² -- and the geodesic angles between z_i and A·g_i·B are summarised.  Every
step runs in the HIP kernels; ``summarize`` is the one host read.
"""
import math

import torch

from .. import _ops
from ..lie_tools import align_rotations, quaternions_to_group_matrix


def _as_matrices(g):
    """Ground truth as matrices: scalar-last quaternions (n,4), as ToyDataset stores them, or
    (n,3,3)."""
    if g.dim() == 2 and g.shape[1] == 4:
        return quaternions_to_group_matrix(g)
    assert g.dim() == 3 and tuple(g.shape[1:]) == (3, 3), \
        f"ground truth must be quaternions (n,4) or matrices (n,3,3), got {tuple(g.shape)}"
    return g


def aligned_errors(Z, G, side='both', rounds=16):
    """Geodesic angles (n,) in radians between Z_i and A·G_i·B after the best alignment."""
    G = _as_matrices(G).to(Z.dtype)
    A, B, _ = align_rotations(Z, G, side=side, rounds=rounds)
    return _ops.so3_angle(Z, A @ G @ B)


def summarize(angles):
    """Mean, median, 90th percentile and maximum of angles (radians) in degrees, as floats:
    one host read."""
    a = torch.rad2deg(angles.detach().double().flatten())
    n = a.numel()
    s = torch.sort(a).values
    # lower median and the ceil(0.9 n)-th order statistic: exact picks, no interpolation
    stats = torch.stack([a.mean(), s[(n - 1) // 2], s[min(n - 1, math.ceil(0.9 * n) - 1)], s[-1]])
    mean, median, p90, mx = stats.tolist()
    return {"mean_deg": mean, "median_deg": median, "p90_deg": p90, "max_deg": mx}


@torch.no_grad()
def posterior_mean_rotations(model, x, batch_size=64):
    """Encode x in chunks and return the posterior mean rotation of every sample, (n,3,3):
    ``rep_group.mu_lie`` for latent mode 'so3', ``quaternions_to_group_matrix(mu)`` for
    'vmfq'; other modes raise (their latent is not a rotation with a known frame)."""
    mode = getattr(model, 'latent_mode', None)
    if mode not in ('so3', 'vmfq'):
        raise ValueError(f"pose evaluation needs latent_mode 'so3' or 'vmfq', got {mode!r}")
    was_training = model.training
    model.eval()
    out = []
    try:
        for i in range(0, x.shape[0], batch_size):
            model.encode(x[i:i + batch_size])
            rep = model.rep_group
            out.append(rep.mu_lie if mode == 'so3' else quaternions_to_group_matrix(rep.mu))
    finally:
        model.train(was_training)
    return torch.cat(out, 0)


def evaluate_poses(model, x, g, batch_size=64, side='both'):
    """Posterior mean rotations of x aligned to the ground truth g (quaternions (n,4) or
    matrices (n,3,3)) -> the dict of ``summarize``."""
    Z = posterior_mean_rotations(model, x, batch_size)
    return summarize(aligned_errors(Z, g.to(Z.device), side=side))
