"""Equivariance loss for the encoder (reference lie_vae/losses/equivariance_loss.py)."""
from math import pi

import torch
import torch.nn as nn

from .. import _ops


class EquivarianceLoss(nn.Module):
    """Equivariance loss for the SO(2) subgroup of rotations about the x axis: an image
    rotated in the plane by theta should encode to g(theta) times the encoding of the
    image.  The rotation, and g · enc − enc_rot squared and summed, are one HIP kernel each
    (``_ops.rotate_images``, ``_ops.equivariance_diff``).

    Deviations from the reference: ``lamb`` is a number or a schedule called
    with ``it`` (the reference calls it unconditionally, so its own default 1.0 fails);
    the per-step ``diffs`` are kept only while a ``log`` is set; ``forward`` takes an
    optional ``theta`` (n,) to inject the angles instead of drawing them."""

    def __init__(self, model, num_samples=None, lamb=1.0, log=None, report_freq=1):
        super().__init__()
        self.model = model
        self.num_samples = num_samples
        self.lamb = lamb
        self.log = log
        self.report_freq = report_freq
        self.diffs = []

    def forward(self, img, encoding, it, theta=None):
        assert encoding.shape[-2:] == (3, 3), "Rotation matrix input required"
        if self.num_samples:
            img, encoding = img[:self.num_samples], encoding[:self.num_samples]
        n = img.shape[0]
        if theta is None:
            theta = torch.rand(n, device=encoding.device) * 2 * pi
        s1 = torch.stack((torch.cos(theta), torch.sin(theta)), 1)

        img_rot = _ops.rotate_images(img, s1)
        img_rot_enc = self.model.encode(img_rot)[0][0]

        diffs = _ops.equivariance_diff(s1, encoding, img_rot_enc)
        if self.log:
            self.diffs.append(diffs.detach())
        mean = diffs.mean()

        lamb = self.lamb(it) if callable(self.lamb) else self.lamb

        if self.log and (it + 1) % self.report_freq == 0:
            agg_diffs = torch.cat(self.diffs)
            self.log.add_scalar('equivariance', agg_diffs.mean(), it + 1)
            self.log.add_scalar('equivariance_lamb', lamb, it + 1)
            self.diffs = []

        return mean * lamb

    @staticmethod
    def rotate(img, theta):
        """img (N, C, H, W) rotated per image by theta (N,), as affine_grid + grid_sample
        with torch's present defaults (align_corners=False)."""
        return _ops.rotate_images(img, torch.stack((torch.cos(theta), torch.sin(theta)), 1))
