"""Encoder regularisers (reference lie_vae/losses/): the SO(2)-equivariance loss and the
pair-continuity loss, on the HIP kernels of csrc/image.hip."""
from .encoder_continuity_loss import EncoderContinuityLoss
from .equivariance_loss import EquivarianceLoss

__all__ = ["EquivarianceLoss", "EncoderContinuityLoss"]
