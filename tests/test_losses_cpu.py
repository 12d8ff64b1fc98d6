"""CPU checks of the encoder regularisers (lie_vae.losses, csrc/image.hip): the API surface
against the reference's names, the six C entry points, their argument checks and the
rotation's launch plan (no device needed: the checks run before any launch), the refusals of
the Python wrappers, the torch restatement in tests/losses_ref.py against the golden file
the reference's own classes wrote, and the trainer's new arguments."""
import ctypes
import inspect

import pytest
import torch
import torch.nn as nn

import losses_ref
from conftest import golden

ENTRY_POINTS = ("lv_rotate_bilinear_fwd", "lv_rotate_plan", "lv_equivariance_diff_fwd",
                "lv_equivariance_diff_bwd", "lv_pair_sqdist_fwd", "lv_pair_sqdist_bwd")


def test_losses_api_matches_reference_names():
    """Class names, constructor arguments and forward parameters of
    lie_vae/losses/equivariance_loss.py:13,22,51 and encoder_continuity_loss.py:9,17; the
    only addition is forward's trailing theta=None."""
    import lie_vae.losses as L
    from lie_vae.losses.encoder_continuity_loss import EncoderContinuityLoss
    from lie_vae.losses.equivariance_loss import EquivarianceLoss
    assert L.EquivarianceLoss is EquivarianceLoss and L.EncoderContinuityLoss is EncoderContinuityLoss

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(EquivarianceLoss.__init__) == [
        ("self", E), ("model", E), ("num_samples", None), ("lamb", 1.0), ("log", None),
        ("report_freq", 1)]
    assert params(EquivarianceLoss.forward) == [
        ("self", E), ("img", E), ("encoding", E), ("it", E), ("theta", None)]
    assert params(EquivarianceLoss.rotate) == [("img", E), ("theta", E)]
    assert isinstance(inspect.getattr_static(EquivarianceLoss, "rotate"), staticmethod)
    assert params(EncoderContinuityLoss.__init__) == [
        ("self", E), ("model", E), ("lamb", 1.0), ("log", None), ("report_freq", 1)]
    assert params(EncoderContinuityLoss.forward) == [("self", E), ("encodings", E), ("it", E)]
    for cls in (EquivarianceLoss, EncoderContinuityLoss):
        assert issubclass(cls, nn.Module)
        assert cls(None).diffs == []


def test_library_exports_the_loss_entry_points():
    from lie_vae import _lib
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
    assert lib.lv_abi_version() == 1
    assert _lib.LV_ROTATE_DIRECT == 1


def test_expand_dim_matches_reference_semantics():
    """experiments/utils.py:82-85: a stride-0 axis of size n at dim (negative dims count from
    the end, after insertion)."""
    from lie_vae.experiments.utils import expand_dim
    x = torch.arange(6.).reshape(2, 3)
    assert expand_dim(x, 4).shape == (4, 2, 3) and expand_dim(x, 4).stride(0) == 0
    assert expand_dim(x, 4, 1).shape == (2, 4, 3)
    assert expand_dim(x, 4, -1).shape == (2, 3, 4)
    assert torch.equal(expand_dim(x, 4, 1)[:, 2], x)


def test_argument_checks_before_any_launch():
    """Bad shapes return LV_ERR_ARG with a message before anything is launched (dummy
    non-null pointers, no device); an empty batch is LV_OK."""
    from lie_vae import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(16)  # never dereferenced: the checks run first
    buf = (ctypes.c_int64 * 4)()

    def refused(rc, word):
        msg = lib.lv_last_error()
        assert rc == -1 and msg and word in msg, (rc, msg)

    rot = lib.lv_rotate_bilinear_fwd
    for C in (0, -1):
        refused(rot(P, P, P, 2, C, 8, 8, 0, 0, None), b"C must")
        refused(lib.lv_rotate_plan(2, C, 8, 8, 0, buf), b"C must")
    for H, W in ((0, 8), (8, 0), (-3, 8)):
        refused(rot(P, P, P, 2, 1, H, W, 0, 0, None), b"H and W")
        refused(lib.lv_rotate_plan(2, 1, H, W, 0, buf), b"H and W")
    for flags in (2, 3, -1):
        refused(rot(P, P, P, 2, 1, 8, 8, 0, flags, None), b"flags")
        refused(lib.lv_rotate_plan(2, 1, 8, 8, flags, buf), b"flags")
    for ac in (2, -1):
        refused(rot(P, P, P, 2, 1, 8, 8, ac, 0, None), b"align_corners")
    refused(rot(P, P, P, -1, 1, 8, 8, 0, 0, None), b"N must")
    refused(rot(None, P, P, 2, 1, 8, 8, 0, 0, None), b"null")
    refused(lib.lv_pair_sqdist_fwd(P, P, 4, 0, None), b"D must")
    refused(lib.lv_pair_sqdist_bwd(P, P, P, 4, -2, None), b"D must")
    refused(lib.lv_pair_sqdist_fwd(P, P, 5, 3, None), b"even")
    refused(lib.lv_pair_sqdist_bwd(P, P, P, 7, 3, None), b"even")
    refused(lib.lv_equivariance_diff_fwd(P, P, P, P, -1, None), b"n must")
    refused(lib.lv_equivariance_diff_bwd(P, P, P, P, P, P, -1, None), b"n must")
    # empty batches: LV_OK, nothing launched
    assert rot(P, P, P, 0, 1, 8, 8, 0, 0, None) == 0
    assert rot(P, P, P, 0, 3, 128, 129, 1, 1, None) == 0
    assert lib.lv_rotate_plan(0, 1, 8, 8, 0, buf) == 0 and buf[1] == 0
    assert lib.lv_equivariance_diff_fwd(P, P, P, P, 0, None) == 0
    assert lib.lv_equivariance_diff_bwd(P, P, P, P, P, P, 0, None) == 0
    assert lib.lv_pair_sqdist_fwd(P, P, 0, 9, None) == 0
    assert lib.lv_pair_sqdist_bwd(P, P, P, 0, 9, None) == 0


def test_rotate_plan_dispatch():
    """The staged path is taken exactly while H·W·4 <= 65,536 bytes and LV_ROTATE_DIRECT is
    clear; its grid is one block per (sample, channel) plane and its LDS the plane."""
    from lie_vae import _lib
    sizes = [(1, 1), (1, 7), (5, 7), (16, 16), (33, 64), (64, 64), (127, 129), (128, 128),
             (128, 129), (129, 128), (160, 128), (1, 16384), (1, 16385), (256, 256)]
    for H, W in sizes:
        for N, C in ((1, 1), (3, 2), (512, 3), (4096, 1)):
            fits = H * W * 4 <= 65536
            p = _lib.rotate_plan(N, C, H, W)
            assert p["staged"] == int(fits), (H, W)
            assert p["threads"] == 256
            if fits:
                assert p["blocks"] == N * C and p["lds_bytes"] == H * W * 4, (N, C, H, W, p)
            else:
                assert p["lds_bytes"] == 0 and 1 <= p["blocks"] <= 65536, (N, C, H, W, p)
            d = _lib.rotate_plan(N, C, H, W, _lib.LV_ROTATE_DIRECT)
            assert d["staged"] == 0 and d["lds_bytes"] == 0 and 1 <= d["blocks"] <= 65536
            # the direct grid covers the four-pixel runs, capped (grid-stride beyond)
            assert d["blocks"] == min(65536, -(-(N * C * -(-H * W // 4)) // 256)), (N, C, H, W, d)
    assert _lib.rotate_plan(3, 1, 64, 64) == {"staged": 1, "blocks": 3, "threads": 256,
                                              "lds_bytes": 16384}
    assert _lib.rotate_plan(1, 1, 128, 128)["staged"] == 1
    assert _lib.rotate_plan(1, 1, 128, 129)["staged"] == 0


def test_cpu_tensors_fail_loudly():
    import lie_vae._ops as ops
    from lie_vae.losses import EncoderContinuityLoss, EquivarianceLoss
    cs = losses_ref.cos_sin(torch.rand(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rotate_images(torch.rand(4, 1, 8, 8), cs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.equivariance_diff(cs, torch.randn(4, 3, 3), torch.randn(4, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pair_sqdist(torch.randn(4, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EquivarianceLoss.rotate(torch.rand(4, 1, 8, 8), torch.rand(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EncoderContinuityLoss(None)(torch.randn(4, 3, 3), 0)


def test_rotate_images_refuses_requires_grad_and_bad_shapes():
    import lie_vae._ops as ops
    cs = losses_ref.cos_sin(torch.rand(4))
    with pytest.raises(RuntimeError, match="no backward"):
        ops.rotate_images(torch.rand(4, 1, 8, 8, requires_grad=True), cs)
    with pytest.raises(AssertionError, match="cs must"):
        ops.rotate_images(torch.rand(4, 1, 8, 8), cs[:3])
    with pytest.raises(AssertionError, match="img must"):
        ops.rotate_images(torch.rand(4, 8, 8), cs)
    with pytest.raises(AssertionError, match="enc and enc_rot"):
        ops.equivariance_diff(cs, torch.randn(4, 3, 3), torch.randn(3, 3, 3))


def test_losses_ref_matches_golden():
    """The restatement against what the reference's own classes computed on the CPU: fp32
    to a few ulp (same ops; the bound leaves room for another CPU's vector width), fp64 within
    the project's forward / gradient tolerances of the fp32 golden values."""
    gold = {k: torch.from_numpy(v) for k, v in golden("losses.npz").items()}
    for tag in ("eqa", "eqb", "eqc"):
        img, theta = gold[f"{tag}_img"], gold[f"{tag}_theta"]
        enc, enc_rot = gold[f"{tag}_enc"], gold[f"{tag}_enc_rot"]
        n = img.shape[0]
        for dt, tol_f, tol_g in ((torch.float32, 2e-6, 2e-6), (torch.float64, 1e-5, 1e-4)):
            cs = losses_ref.cos_sin(theta).to(dt)
            rot = losses_ref.rotate(img.to(dt), cs)
            assert losses_ref.normwise(rot, gold[f"{tag}_img_rot"]).max() <= tol_f
            gout = torch.full((n,), float(gold[f"{tag}_lamb"]) / n, dtype=dt)
            diffs, (ge, gr) = losses_ref.grads(
                lambda a, b: losses_ref.equivariance_diffs(cs, a, b),
                [enc.to(dt), enc_rot.to(dt)], gout)
            assert losses_ref.normwise(diffs[None], gold[f"{tag}_diffs"][None]).max() <= tol_f
            loss = diffs.mean() * float(gold[f"{tag}_lamb"])
            assert abs(float(loss) - float(gold[f"{tag}_loss"])) <= tol_f * abs(float(gold[f"{tag}_loss"]))
            assert losses_ref.normwise(ge, gold[f"{tag}_g_enc"]).max() <= tol_g
            assert losses_ref.normwise(gr, gold[f"{tag}_g_enc_rot"]).max() <= tol_g
    for tag in ("cta", "ctb"):
        enc = gold[f"{tag}_enc"]
        n = enc.shape[0] // 2
        for dt, tol_f, tol_g in ((torch.float32, 2e-6, 2e-6), (torch.float64, 1e-5, 1e-4)):
            gout = torch.full((n,), 0.7 / n, dtype=dt)
            diffs, (ge,) = losses_ref.grads(losses_ref.pair_sqdist, [enc.to(dt)], gout)
            assert losses_ref.normwise(diffs[None], gold[f"{tag}_diffs"][None]).max() <= tol_f
            assert abs(float(diffs.mean()) * 0.7 - float(gold[f"{tag}_loss"])) <= tol_f * float(gold[f"{tag}_loss"])
            sched = float(diffs.mean()) * (0.5 + 0.25 * int(gold[f"{tag}_it"]))
            assert abs(sched - float(gold[f"{tag}_loss_sched"])) <= tol_f * float(gold[f"{tag}_loss_sched"])
            assert losses_ref.normwise(ge.reshape(2 * n, -1), gold[f"{tag}_g_enc"].reshape(2 * n, -1)).max() <= tol_g


class _TinyVAE(nn.Module):
    """Torch-only stand-in with the VAE's contract (as tests/test_dp_gloo.py's)."""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(nn.Linear(12, 16), nn.Tanh(), nn.Linear(16, 6))
        self.rep_group = nn.Linear(6, 6)
        self.dec = nn.Linear(3, 12)

    def forward(self, x, n=1, eps=None):
        h = self.rep_group(self.encoder(x))
        mu, logs = h[:, :3], h[:, 3:]
        z = mu + (eps if eps is not None else 0.0) * logs.exp()
        self._kl = 0.5 * (mu.square() + (2 * logs).exp() - 2 * logs - 1).sum(-1)
        return self.dec(z)

    def recon_loss(self, x_recon, x):
        return (x_recon - x).square().sum(-1)

    def elbo(self, x, n=1, eps=None):
        x_recon = self.forward(x, n, eps)
        return self.recon_loss(x_recon, x), self._kl, [self._kl]


def test_dptrainer_default_step_unchanged_and_new_arguments():
    """Without the new arguments _loss is the ELBO of unsupervised.py:85-88 and no loss
    module exists; with them the modules are built as unsupervised.py:44-56 builds them; and
    capture() refuses a non-constant schedule for either before touching a device."""
    from lie_vae.experiments import train_dp
    from lie_vae.losses import EncoderContinuityLoss, EquivarianceLoss
    sig = list(inspect.signature(train_dp.DPTrainer.__init__).parameters.values())
    assert [(p.name, p.default) for p in sig[-2:]] == [("equivariance_lamb", None),
                                                      ("encoder_continuity_lamb", None)]
    torch.manual_seed(3)
    model = _TinyVAE()
    tr = train_dp.DPTrainer(model, lr=1e-2)
    assert tr.equivariance_loss is None and tr.encoder_continuity_loss is None
    x, eps = torch.randn(8, 12), torch.randn(8, 3)
    loss, recon, kl = tr._loss(x, eps, 0.5)
    r2, k2, _ = model.elbo(x, eps=eps)
    assert torch.equal(loss, (r2 + 0.5 * k2).mean()) and torch.equal(recon, r2) and torch.equal(kl, k2)

    ramp = train_dp.LinearSchedule(0.0, 1.0, 1, 10)
    tr = train_dp.DPTrainer(_TinyVAE(), lr=1e-2, equivariance_lamb=ramp, encoder_continuity_lamb=0.25)
    assert isinstance(tr.equivariance_loss, EquivarianceLoss) and tr.equivariance_loss.lamb is ramp
    assert isinstance(tr.encoder_continuity_loss, EncoderContinuityLoss)
    assert tr.encoder_continuity_loss.lamb == 0.25
    assert tr.equivariance_loss.model is tr.model and tr.equivariance_loss.log is None

    for kw, word in (({"equivariance_lamb": ramp}, "equivariance_lamb"),
                     ({"encoder_continuity_lamb": ramp}, "encoder_continuity_lamb"),
                     ({"equivariance_lamb": 1.0, "encoder_continuity_lamb": lambda it: 0.1 * it},
                      "encoder_continuity_lamb")):
        tr = train_dp.DPTrainer(_TinyVAE(), lr=1e-2, graph=True, **kw)
        with pytest.raises(ValueError, match=f"constant {word}"):
            tr.capture(torch.randn(4, 12))
    # the beta rule is as before
    tr = train_dp.DPTrainer(_TinyVAE(), lr=1e-2, graph=True, beta=ramp)
    with pytest.raises(ValueError, match="constant, non-zero beta"):
        tr.capture(torch.randn(4, 12))
