"""The VAE that wires encoder -> SO(3) latent -> action decoder (reference
lie_vae/experiments/vae.py:16-204), with the *intended* behaviour of the two shipped
defects: ``encode`` treats the never-assigned ``r_callback`` as
None, and ``decode`` calls the decoder with the angles only (ignoring z_content).

Encoder/deconv are dense convs on PyTorch-ROCm; every op between them — mean map,
N0 sample, z = mu exp(v), Euler extraction, Wigner-D action, the 21-term log-density —
runs in the HIP kernels of liblievae_hip.so.
"""
import numpy as np
import torch
import torch.nn as nn

from ..decoders import ActionNet, MLPNet
from ..lie_tools import group_matrix_to_eazyz, quaternions_to_eazyz, vector_to_eazyz
from ..reparameterize import (AlgebraMean, N0reparameterize, Nreparameterize, QuaternionMean,
                              S2S1Mean, S2S2Mean, SO3reparameterize, Sreparameterize, SVDMean)
from ..utils import logsumexp
from .nets import MLP, ConvNet, ConvNetBN, DeconvNet, Flatten

# 'svd' is an extension: a 9-D linear head projected onto SO(3)
_MEANS = {'alg': AlgebraMean, 'q': QuaternionMean, 's2s1': S2S1Mean, 's2s2': S2S2Mean,
          'svd': SVDMean}

# Under reduced-precision autocast, the latent heads -- the encoder's last (4x4 -> 1x1)
# GEMM conv and the mean / sigma linears (reparameterize.py:148-197) -- compute in fp32:
# 0 = off (all autocast), 1 = the rep_group heads, 2 = the heads and the encoder's last
# conv.  A bf16 rounding of the mean map's output is a 2^-9 perturbation of the S2S2
# Gram-Schmidt's input, whose near-parallel pairs amplify it; the layers
# are (512 x 6400) x (6400 x 10) and (10 x 6) GEMMs, so fp32 costs nothing measurable.
# Over 50 config-3 steps (s2s2) the bf16 trajectory's distance from the fp32 one
# (rep_group: cos -0.15 / 0.75 / 0.66 for modes 0 / 1 / 2, against 0.30 for fp32 itself
# under a 2^-9 input perturbation; profiles/r06_bf16_trajectory_s2s2.json): mode 1.
AMP_FP32_HEADS = 1


class VAE(nn.Module):
    def __init__(self, *, latent_mode, decoder_mode, degrees=6, deconv_hidden=50,
                 encode_mode='conv', deconv_mode='deconv', rep_copies=10, batch_norm=True,
                 rgb=False, mean_mode='alg', group_reparam_in_dims=10, normal_dims=3,
                 deterministic=False, item_rep=None, wigner_transpose=False, mlp_layers=3,
                 mlp_hidden=50, mlp_activation=nn.ReLU, fixed_sigma=None, fused_decode=True):
        super().__init__()
        # decode z = mu·exp(v) with the one-launch fused kernel when z is the latest
        # SO(3) sample (same function, fewer launches)
        self.fused_decode = fused_decode
        self.latent_mode = latent_mode
        self.decoder_mode = decoder_mode
        self.r_callback = None
        matrix_dims = (degrees + 1) ** 2
        self.out_shape = (matrix_dims, rep_copies) if deconv_mode == 'toy' else \
            (3 if rgb else 1, 64, 64)

        if latent_mode == 'normal':
            if decoder_mode != 'mlp' and normal_dims != 3:
                raise ValueError('Normal Action must be 3 dim')
            group_reparam_in_dims = max(group_reparam_in_dims, normal_dims)

        if encode_mode == 'conv':
            self.encoder = (ConvNetBN if batch_norm else ConvNet)(group_reparam_in_dims, rgb=rgb)
        elif encode_mode == 'toy':
            self.encoder = nn.Sequential(
                Flatten(), MLP(matrix_dims * rep_copies, group_reparam_in_dims, 100, 2,
                               activation=mlp_activation))
        else:
            raise ValueError('Wrong encode mode')

        if latent_mode == 'so3':
            if mean_mode not in _MEANS:
                raise ValueError('Wrong mean mode')
            normal = N0reparameterize(group_reparam_in_dims, z_dim=3, fixed_sigma=fixed_sigma)
            self.rep_group = SO3reparameterize(normal, _MEANS[mean_mode](group_reparam_in_dims),
                                               k=10)
            group_dims = 9
        elif latent_mode == 'normal':
            self.rep_group = Nreparameterize(group_reparam_in_dims, normal_dims)
            group_dims = normal_dims
        elif latent_mode in ('vmf', 'vmfq'):
            self.rep_group = Sreparameterize(group_reparam_in_dims, 4)
            group_dims = 4
        else:
            raise ValueError('Wrong latent mode')
        if deterministic:
            self.rep_group.deterministic()
        self.reparameterize = nn.ModuleList([self.rep_group])

        if deconv_mode == 'deconv':
            deconv = DeconvNet(matrix_dims * rep_copies, deconv_hidden, rgb=rgb)
        elif deconv_mode == 'toy':
            deconv = nn.Sequential()
        else:
            raise RuntimeError()
        if decoder_mode == 'action':
            self.decoder = ActionNet(degrees=degrees, deconv=deconv, rep_copies=rep_copies,
                                     item_rep=item_rep, transpose=wigner_transpose)
        elif decoder_mode == 'mlp':
            self.decoder = MLPNet(degrees=degrees, in_dims=group_dims, deconv=deconv,
                                  rep_copies=rep_copies, layers=mlp_layers,
                                  hidden_dims=mlp_hidden, activation=mlp_activation)
        else:
            raise RuntimeError()

    def encode(self, x, n=1, eps=None):
        amp = torch.is_autocast_enabled(x.device.type) and AMP_FP32_HEADS > 0
        if amp and AMP_FP32_HEADS > 1 and isinstance(self.encoder, nn.Sequential):
            mods = list(self.encoder)
            h = x
            for m in mods[:-2]:
                h = m(h)
            with torch.autocast(x.device.type, enabled=False):
                h = h.float()
                for m in mods[-2:]:
                    h = m(h)
        else:
            h = self.encoder(x)
        if amp:
            with torch.autocast(x.device.type, enabled=False):
                return self._reparam(h.float(), n, eps)
        return self._reparam(h, n, eps)

    def _reparam(self, h, n, eps):
        if self.r_callback is not None:
            return [r(f(h), n) for r, f in zip(self.reparameterize, self.r_callback)]
        if eps is not None:
            # the vMF module's injected noise is (n, B, 6·trials + 3) and is named `noise`
            return [r(h, n, noise=eps) if isinstance(r, Sreparameterize) else r(h, n, eps=eps)
                    for r in self.reparameterize]
        return [r(h, n) for r in self.reparameterize]

    def kl(self):
        return [r.kl() for r in self.reparameterize]

    def forward(self, x, n=1, eps=None):
        z = self.encode(x, n=n, eps=eps)
        self.z = z
        return self.decode(*z)

    def elbo(self, x, n=1, eps=None):
        x_recon = self.forward(x, n, eps=eps)
        kl = self.kl()
        kl_summed = torch.sum(torch.stack(kl, -1), -1)
        return self.recon_loss(x_recon, x), kl_summed, kl

    def log_likelihood(self, x, n=1, eps=None):
        """Importance-weighted log-likelihood (vae.py:164-171), averaged over the batch.

        The reference evaluates it one image at a time with n = 500 (main.py:134-139);
        any batch gives the same per-image terms, so a caller can evaluate many test
        images per launch.  ``eps`` (n, B, 3) optionally injects the latent noise (the
        reference always draws it; ``None`` keeps that)."""
        x_recon = self.forward(x, n, eps=eps)
        log_p_z = torch.cat([r.log_prior() for r in self.reparameterize], -1).to(x.device)
        log_q_z_x = torch.cat([r.log_posterior() for r in self.reparameterize], -1).to(x.device)
        log_p_x_z = -self.recon_loss(x_recon, x)
        return (logsumexp(log_p_x_z + log_p_z - log_q_z_x, dim=0) - np.log(n)).mean()

    def _fusable(self, z_pose):
        """z_pose is the SO(3) sample mu·exp(v) the latent module just drew (not its means),
        and the decoder is the action decoder: decode it from (mu, v) in one launch."""
        rep = getattr(self, 'rep_group', None)
        return (self.fused_decode and self.decoder_mode == 'action'
                and self.latent_mode == 'so3' and isinstance(rep, SO3reparameterize)
                and z_pose is rep.z and not rep.return_means and rep.v is not None
                and rep.v.dim() == 3 and tuple(rep.v.shape[:2]) == tuple(z_pose.shape[:2]))

    def decode(self, z_pose, z_content=None):
        batch_dims = z_pose.shape[:2]
        if self._fusable(z_pose):
            rep = self.rep_group
            n, B = batch_dims
            mu = rep.mu_lie.expand(n, -1, -1, -1).reshape(-1, 3, 3)
            x_recon = self.decoder.forward_fused(mu, rep.v.reshape(-1, 3))
            return x_recon.reshape(*batch_dims, *self.out_shape)
        z_pose = z_pose.reshape(-1, *z_pose.shape[2:])
        if self.decoder_mode == 'action':
            if self.latent_mode in ('so3', 'so3f'):
                angles = group_matrix_to_eazyz(z_pose)
            elif self.latent_mode in ('normal', 'vmf'):
                angles = vector_to_eazyz(z_pose)
            elif self.latent_mode == 'vmfq':
                angles = quaternions_to_eazyz(z_pose)
            else:
                raise RuntimeError()
            x_recon = self.decoder(angles)
        elif self.decoder_mode == 'mlp':
            x_recon = self.decoder(z_pose)
        else:
            raise RuntimeError()
        return x_recon.reshape(*batch_dims, *self.out_shape)

    def recon_loss(self, x_recon, x):
        """Summed squared error over (C, H, W) (vae.py:199-204)."""
        x = x.expand_as(x_recon)
        loss = (x_recon - x) ** 2
        for _ in range(len(self.out_shape)):
            loss = loss.sum(-1)
        return loss
