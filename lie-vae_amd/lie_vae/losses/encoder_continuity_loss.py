"""Continuity loss for the encoder (reference lie_vae/losses/encoder_continuity_loss.py)."""
import torch
import torch.nn as nn

from .. import _ops


class EncoderContinuityLoss(nn.Module):
    """Encoder continuity loss for nearby input pairs: adjacent rows of the batch are a
    pair, and the loss is lamb(it) times the mean squared distance of their encodings
    (one HIP kernel each way, ``_ops.pair_sqdist``).

    ``lamb`` is a number or a schedule called with ``it``.  With a ``log`` the mean of the
    per-pair distances since the last report and the current lamb are written with
    ``log.add_scalar`` whenever ``(it + 1) % report_freq == 0``; without one nothing is
    kept (the reference appends every step's distances to ``self.diffs`` forever)."""

    def __init__(self, model, lamb=1.0, log=None, report_freq=1):
        super().__init__()
        self.model = model
        self.lamb = lamb
        self.log = log
        self.report_freq = report_freq
        self.diffs = []

    def forward(self, encodings, it):
        n = encodings.shape[0] // 2
        diffs = _ops.pair_sqdist(encodings.reshape(2 * n, -1))
        if self.log:
            self.diffs.append(diffs.detach())
        mean = diffs.mean()

        lamb = self.lamb(it) if callable(self.lamb) else self.lamb

        if self.log and (it + 1) % self.report_freq == 0:
            agg_diffs = torch.cat(self.diffs)
            self.log.add_scalar('encoder_continuity', agg_diffs.mean(), it + 1)
            self.log.add_scalar('encoder_continuity_lamb', lamb, it + 1)
            self.diffs = []

        return mean * lamb
