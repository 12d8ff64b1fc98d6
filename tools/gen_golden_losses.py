"""Generate tests/golden/losses.npz by running the REFERENCE's own EquivarianceLoss and
EncoderContinuityLoss on the CPU (build container only, like oracle/gen_golden.py, whose
stub packages this script reuses).

Run:  python tools/gen_golden_losses.py

The model is a stub whose ``encode`` records the rotated batch it is given and returns a
fixed tensor; theta is recovered by reseeding the generator the loss draws from.  The file
holds data only: inputs, angles, rotated images, encodings, per-sample diffs, loss values
and autograd gradients.
"""
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.gen_golden import _install_stubs, _np  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "losses.npz")


class StubModel:
    """encode(img) -> [z] with z[0] the recorded encoding of the rotated batch."""

    def __init__(self, enc_rot):
        self.enc_rot = enc_rot
        self.seen = None

    def encode(self, img):
        self.seen = img.detach().clone()
        return [self.enc_rot[None]]


def lamb_schedule(it):
    return 0.5 + 0.25 * it


def smooth_plane(h, w):
    y, x = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    return 0.5 + 0.3 * torch.sin(3.0 * x + 1.0) * torch.cos(2.0 * y - 0.5) + 0.2 * x * y


def main():
    _install_stubs()
    import lie_vae.experiments  # noqa: F401  (first: the reference's import cycle)
    from lie_vae.losses.encoder_continuity_loss import EncoderContinuityLoss
    from lie_vae.losses.equivariance_loss import EquivarianceLoss

    g = torch.Generator().manual_seed(2024)
    out = {}
    images = {"eqa": torch.rand(4, 1, 16, 16, generator=g),
              "eqb": torch.rand(2, 3, 16, 16, generator=g),
              "eqc": torch.stack((torch.rand(1, 64, 64, generator=g), smooth_plane(64, 64)[None]))}
    for k, (tag, img) in enumerate(images.items()):
        n, it, seed = img.shape[0], 3 + k, 100 + k
        enc = torch.randn(n, 3, 3, generator=g).requires_grad_(True)
        enc_rot = torch.randn(n, 3, 3, generator=g).requires_grad_(True)
        model = StubModel(enc_rot)
        loss_mod = EquivarianceLoss(model, lamb=lamb_schedule)
        torch.manual_seed(seed)
        loss = loss_mod(img, enc, it)
        torch.manual_seed(seed)
        theta = torch.rand(n) * 2 * math.pi
        loss.backward()
        assert torch.equal(model.seen, EquivarianceLoss.rotate(img, theta))
        out.update({f"{tag}_img": img, f"{tag}_theta": theta, f"{tag}_img_rot": model.seen,
                    f"{tag}_enc": enc, f"{tag}_enc_rot": enc_rot,
                    f"{tag}_diffs": loss_mod.diffs[0], f"{tag}_loss": loss,
                    f"{tag}_it": torch.tensor(it), f"{tag}_lamb": torch.tensor(lamb_schedule(it)),
                    f"{tag}_g_enc": enc.grad, f"{tag}_g_enc_rot": enc_rot.grad})

    for tag, shape in (("cta", (8, 3, 3)), ("ctb", (6, 5))):
        enc = torch.randn(*shape, generator=g).requires_grad_(True)
        num = EncoderContinuityLoss(None, lamb=0.7)
        loss = num(enc, 5)
        loss.backward()
        sched = EncoderContinuityLoss(None, lamb=lamb_schedule)
        loss_s = sched(enc.detach(), 5)
        out.update({f"{tag}_enc": enc, f"{tag}_diffs": num.diffs[0], f"{tag}_loss": loss,
                    f"{tag}_loss_sched": loss_s, f"{tag}_it": torch.tensor(5),
                    f"{tag}_g_enc": enc.grad})

    np.savez(OUT, **{k: _np(v) for k, v in out.items()})
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")
    assert os.path.getsize(OUT) < 256 * 1024


if __name__ == "__main__":
    main()
