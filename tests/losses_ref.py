"""Torch restatement of the encoder regularisers' arithmetic (reference
lie_vae/losses/equivariance_loss.py, encoder_continuity_loss.py, lie_tools.py:67-78), in
the dtype and on the device of its inputs: fp32 as the reference runs it, fp64 as the
tests' yardstick.  tests/test_losses_cpu.py pins it to tests/golden/losses.npz, which the
reference's own classes wrote (tools/gen_golden_losses.py)."""
import torch
import torch.nn.functional as F


def cos_sin(theta):
    return torch.stack((torch.cos(theta), torch.sin(theta)), 1)


def rotate(img, cs, align_corners=False):
    """EquivarianceLoss.rotate with (cos, sin) given: affine_grid + grid_sample."""
    c, s = cs[:, 0], cs[:, 1]
    zero = torch.zeros_like(c)
    affine = torch.stack([c, -s, zero, s, c, zero], 1).view(-1, 2, 3)
    grid = F.affine_grid(affine, list(img.size()), align_corners=align_corners)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros",
                         align_corners=align_corners)


def rotation_about_x(cs):
    """s2s1rodrigues((1, 0, 0), cs) = I + sin K + (1 - cos) K@K."""
    K = cs.new_tensor([[0., 0., 0.], [0., 0., -1.], [0., 1., 0.]])
    eye = torch.eye(3, device=cs.device, dtype=cs.dtype)
    return eye + cs[:, 1, None, None] * K + (1. - cs[:, 0])[:, None, None] * (K @ K)


def equivariance_diffs(cs, enc, enc_rot):
    n = enc.shape[0]
    return (rotation_about_x(cs).bmm(enc) - enc_rot).pow(2).reshape(n, -1).sum(-1)


def pair_sqdist(enc):
    n = enc.shape[0] // 2
    e = enc.reshape(n, 2, -1)
    return (e[:, 0] - e[:, 1]).pow(2).reshape(n, -1).sum(-1)


def normwise(y, ref):
    """||y - ref|| / ||ref|| per leading index, in fp64."""
    y = y.detach().double().cpu().reshape(y.shape[0], -1)
    ref = ref.detach().double().cpu().reshape(ref.shape[0], -1)
    return (y - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)


def grads(fn, inputs, gout):
    """(fn(*inputs) * gout).sum() differentiated with respect to every input."""
    xs = [x.detach().clone().requires_grad_(True) for x in inputs]
    y = fn(*xs)
    (y * gout).sum().backward()
    return y.detach(), [x.grad for x in xs]
