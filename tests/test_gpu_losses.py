"""GPU tests of the encoder regularisers (csrc/image.hip through lie_vae._ops and
lie_vae.losses): the rotation against an fp64 restatement and on exact operands, the two
dispatch paths against each other, the loss kernels against the golden file and fp64
autograd, the modules' values and reporting cadence, one trainer step, and graph replay.

Tolerances are DESIGN.md §2's: forward 1e-5 and gradients 1e-4, normwise per sample (per
image for the rotation, where an image may instead stay within twice the error the fp32
torch restatement itself has against fp64 on that image)."""
import copy
import functools
import math

import pytest
import torch

import losses_ref
from conftest import golden

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-5, 1e-4
# (N, C, H, W): the reference's 64x64 planes at C = 1 and 3, odd sizes that are no multiple
# of the four-pixel run, H != W, one pixel, and a plane over 64 KB (direct path only)
SHAPES = [(3, 1, 64, 64), (2, 3, 64, 64), (5, 2, 5, 7), (2, 1, 33, 64), (1, 1, 1, 1),
          (1, 1, 160, 128)]
SQUARE = [s for s in SHAPES if s[2] == s[3]]
FITS = [s for s in SHAPES if s[2] * s[3] * 4 <= 65536]


def _image(shape, kind, seed=0):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + N)
    if kind == "noise":
        return torch.rand(N, C, H, W, generator=g)
    y = torch.linspace(-1, 1, H)[:, None]
    x = torch.linspace(-1, 1, W)[None, :]
    ph = torch.rand(N, C, 1, 1, generator=g) * 3
    return 0.5 + 0.3 * torch.sin(3.0 * x + ph) * torch.cos(2.0 * y - ph) + 0.2 * x * y


@functools.lru_cache(maxsize=None)
def _case(shape, kind, align):
    """Inputs and the CPU references of one rotation case, computed once and shared."""
    img = _image(shape, kind)
    g = torch.Generator().manual_seed(shape[2] * 131 + shape[3] + int(align))
    cs = losses_ref.cos_sin(torch.rand(shape[0], generator=g) * 2 * math.pi)
    ref64 = losses_ref.rotate(img.double(), cs.double(), align)
    ref32 = losses_ref.rotate(img, cs, align)
    return img, cs, ref64, ref32


def _check_rotation(y, ref64, ref32, what):
    err = losses_ref.normwise(y, ref64)
    err32 = losses_ref.normwise(ref32, ref64)
    print(f"{what}: normwise err max {err.max():.3e} (fp32 torch restatement {err32.max():.3e})")
    ok = (err <= FWD_TOL) | (err <= 2 * err32)
    assert ok.all(), (what, err.tolist(), err32.tolist())


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rotation_vs_fp64(gpu_device, shape, kind, align):
    import lie_vae._ops as ops
    img, cs, ref64, ref32 = _case(shape, kind, align)
    y = ops.rotate_images(img.to(gpu_device), cs.to(gpu_device), align_corners=align)
    assert y.shape == img.shape and y.dtype == torch.float32
    _check_rotation(y, ref64, ref32, f"{shape} {kind} align={align}")


def test_rotation_golden_images(gpu_device):
    """The images the reference's own EquivarianceLoss.rotate produced, to the same bound
    (the yardstick stays the fp64 restatement at the golden angles)."""
    import lie_vae._ops as ops
    from lie_vae.losses import EquivarianceLoss
    gold = {k: torch.from_numpy(v) for k, v in golden("losses.npz").items()}
    for tag in ("eqa", "eqb", "eqc"):
        img, theta, want = gold[f"{tag}_img"], gold[f"{tag}_theta"], gold[f"{tag}_img_rot"]
        cs = losses_ref.cos_sin(theta)
        ref64 = losses_ref.rotate(img.double(), cs.double())
        y = ops.rotate_images(img.to(gpu_device), cs.to(gpu_device))
        _check_rotation(y, ref64, want, f"golden {tag}")
        # and against the golden images themselves, each within the bound of fp64
        gap = losses_ref.normwise(y, want)
        own = losses_ref.normwise(want, ref64)
        assert (gap <= FWD_TOL + own).all(), (tag, gap.tolist(), own.tolist())
        # the static method draws cos / sin on the device
        z = EquivarianceLoss.rotate(img.to(gpu_device), theta.to(gpu_device))
        _check_rotation(z, ref64, want, f"golden {tag} via EquivarianceLoss.rotate")


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rotation_exact_operands(gpu_device, shape, align):
    """(c, s) = (1, 0) is the identity and (-1, 0) the half turn at any size, (0, +-1) the
    quarter turns of a square image: exact source positions, so the pixels are copied bit for
    bit (a property of this kernel; torch's CPU path is not exact here)."""
    import lie_vae._ops as ops
    N = shape[0]
    img = _image(shape, "noise", seed=1)
    x = img.to(gpu_device)

    def run(c, s):
        cs = torch.tensor([[c, s]], dtype=torch.float32).expand(N, 2).contiguous()
        return cs, ops.rotate_images(x, cs.to(gpu_device), align_corners=align).cpu()

    _, y = run(1.0, 0.0)
    assert torch.equal(y, img)
    _, y = run(-1.0, 0.0)
    assert torch.equal(y, img.flip(-1, -2))
    if shape in SQUARE:
        for s in (1.0, -1.0):
            cs, y = run(0.0, s)
            ref = losses_ref.rotate(img, cs, align)
            dist = [float((ref - torch.rot90(img, k, (-2, -1))).norm()) for k in range(4)]
            k = min(range(4), key=dist.__getitem__)
            assert dist[k] <= 1e-4 * max(float(ref.norm()), 1e-30), dist
            if shape[2] > 1:
                assert k in (1, 3)
            assert torch.equal(y, torch.rot90(img, k, (-2, -1))), (s, k)


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("shape", FITS, ids=lambda s: "x".join(map(str, s)))
def test_rotation_paths_bitwise_equal(gpu_device, shape, align):
    """The staged (LDS) and direct (global-memory taps) paths share the tap arithmetic; so do
    the 16-byte and the one-pixel variants (taken for a tensor that is not 16-byte aligned)."""
    import lie_vae._ops as ops
    from lie_vae import _lib
    assert _lib.rotate_plan(*shape)["staged"] == 1
    assert _lib.rotate_plan(*shape, _lib.LV_ROTATE_DIRECT)["staged"] == 0
    img, cs, _, _ = _case(shape, "noise", align)
    x, c = img.to(gpu_device), cs.to(gpu_device)
    staged = ops.rotate_images(x, c, align_corners=align)
    direct = ops.rotate_images(x, c, align_corners=align, flags=_lib.LV_ROTATE_DIRECT)
    assert torch.equal(staged, direct)
    # the same planes at a 4-byte offset: contiguous, not 16-byte aligned
    buf = torch.empty(x.numel() + 1, device=gpu_device)
    shifted = buf[1:].view_as(x).copy_(x)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    assert torch.equal(ops.rotate_images(shifted, c, align_corners=align), staged)
    assert torch.equal(ops.rotate_images(shifted, c, align_corners=align,
                                         flags=_lib.LV_ROTATE_DIRECT), staged)


def test_rotation_empty_batch(gpu_device):
    import lie_vae._ops as ops
    y = ops.rotate_images(torch.empty(0, 3, 8, 8, device=gpu_device),
                          torch.empty(0, 2, device=gpu_device))
    assert y.shape == (0, 3, 8, 8)


# ---------------------------------------------------------------- loss kernels
def _per_sample_ok(y, ref, tol, what):
    err = losses_ref.normwise(y.reshape(y.shape[0], -1), ref.reshape(ref.shape[0], -1))
    print(f"{what}: normwise err max {err.max():.3e}")
    assert (err <= tol).all(), (what, float(err.max()))


def test_loss_kernels_vs_golden(gpu_device):
    """Forward values and both gradients of the loss the reference's classes computed on the
    CPU (loss = mean(diffs) · lamb, so gdiffs = lamb / n)."""
    import lie_vae._ops as ops
    gold = {k: torch.from_numpy(v) for k, v in golden("losses.npz").items()}
    for tag in ("eqa", "eqb", "eqc"):
        cs = losses_ref.cos_sin(gold[f"{tag}_theta"]).to(gpu_device)
        enc = gold[f"{tag}_enc"].to(gpu_device).requires_grad_(True)
        enc_rot = gold[f"{tag}_enc_rot"].to(gpu_device).requires_grad_(True)
        diffs = ops.equivariance_diff(cs, enc, enc_rot)
        loss = diffs.mean() * float(gold[f"{tag}_lamb"])
        loss.backward()
        _per_sample_ok(diffs[:, None], gold[f"{tag}_diffs"][:, None], FWD_TOL, f"{tag} diffs")
        assert float(loss) == pytest.approx(float(gold[f"{tag}_loss"]), rel=FWD_TOL)
        _per_sample_ok(enc.grad, gold[f"{tag}_g_enc"], GRAD_TOL, f"{tag} g_enc")
        _per_sample_ok(enc_rot.grad, gold[f"{tag}_g_enc_rot"], GRAD_TOL, f"{tag} g_enc_rot")
    for tag in ("cta", "ctb"):
        enc = gold[f"{tag}_enc"].to(gpu_device).requires_grad_(True)
        rows = enc.shape[0]
        diffs = ops.pair_sqdist(enc.reshape(rows, -1))
        loss = diffs.mean() * 0.7
        loss.backward()
        _per_sample_ok(diffs[:, None], gold[f"{tag}_diffs"][:, None], FWD_TOL, f"{tag} diffs")
        assert float(loss) == pytest.approx(float(gold[f"{tag}_loss"]), rel=FWD_TOL)
        _per_sample_ok(enc.grad.reshape(rows, -1), gold[f"{tag}_g_enc"].reshape(rows, -1), GRAD_TOL,
                       f"{tag} g_enc")


@pytest.mark.parametrize("n", [1, 7, 1000])
def test_equivariance_diff_vs_fp64_autograd(gpu_device, n):
    import lie_vae._ops as ops
    g = torch.Generator().manual_seed(40 + n)
    cs = losses_ref.cos_sin(torch.rand(n, generator=g) * 2 * math.pi)
    enc, enc_rot = torch.randn(n, 3, 3, generator=g), torch.randn(n, 3, 3, generator=g)
    gdiffs = torch.randn(n, generator=g)  # non-uniform
    ref, (ge, gr) = losses_ref.grads(
        lambda a, b: losses_ref.equivariance_diffs(cs.double(), a, b),
        [enc.double(), enc_rot.double()], gdiffs.double())
    runs = []
    for _ in range(2):
        a = enc.to(gpu_device).requires_grad_(True)
        b = enc_rot.to(gpu_device).requires_grad_(True)
        y = ops.equivariance_diff(cs.to(gpu_device), a, b)
        (y * gdiffs.to(gpu_device)).sum().backward()
        runs.append((y.detach().cpu(), a.grad.cpu(), b.grad.cpu()))
    y, ga, gb = runs[0]
    _per_sample_ok(y[:, None], ref[:, None], FWD_TOL, f"equivariance diffs n={n}")
    _per_sample_ok(ga, ge, GRAD_TOL, f"equivariance g_enc n={n}")
    _per_sample_ok(gb, gr, GRAD_TOL, f"equivariance g_enc_rot n={n}")
    for u, v in zip(*runs):  # bitwise reproducible run to run
        assert torch.equal(u, v)


@pytest.mark.parametrize("D", [1, 9, 37])
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_pair_sqdist_vs_fp64_autograd(gpu_device, n, D):
    import lie_vae._ops as ops
    g = torch.Generator().manual_seed(50 + n + D)
    enc = torch.randn(2 * n, D, generator=g)
    gdiffs = torch.randn(n, generator=g)
    ref, (ge,) = losses_ref.grads(losses_ref.pair_sqdist, [enc.double()], gdiffs.double())
    runs = []
    for _ in range(2):
        a = enc.to(gpu_device).requires_grad_(True)
        y = ops.pair_sqdist(a)
        (y * gdiffs.to(gpu_device)).sum().backward()
        runs.append((y.detach().cpu(), a.grad.cpu()))
    y, ga = runs[0]
    assert y.shape == (n,) and ga.shape == (2 * n, D)
    _per_sample_ok(y[:, None], ref[:, None], FWD_TOL, f"pair diffs n={n} D={D}")
    # per pair: both rows of a pair carry the same gradient up to sign
    _per_sample_ok(ga.reshape(n, 2 * D), ge.reshape(n, 2 * D), GRAD_TOL, f"pair g_enc n={n} D={D}")
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_loss_kernels_empty_batch(gpu_device):
    import lie_vae._ops as ops
    e = torch.empty(0, 3, 3, device=gpu_device)
    assert ops.equivariance_diff(torch.empty(0, 2, device=gpu_device), e, e).shape == (0,)
    assert ops.pair_sqdist(torch.empty(0, 9, device=gpu_device)).shape == (0,)


# ---------------------------------------------------------------- modules
class _StubModel:
    """encode(img) -> [z] with z[0] a recorded tensor (as tools/gen_golden_losses.py's)."""

    def __init__(self, enc_rot):
        self.enc_rot, self.seen = enc_rot, None

    def encode(self, img):
        self.seen = img
        return [self.enc_rot[None]]


class _StubLog:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, float(value), step))


def _schedule(it):
    return 0.5 + 0.25 * it


def test_modules_vs_golden_losses(gpu_device):
    from lie_vae.losses import EncoderContinuityLoss, EquivarianceLoss
    gold = {k: torch.from_numpy(v) for k, v in golden("losses.npz").items()}
    for tag in ("eqa", "eqb", "eqc"):
        model = _StubModel(gold[f"{tag}_enc_rot"].to(gpu_device))
        mod = EquivarianceLoss(model, lamb=_schedule)
        loss = mod(gold[f"{tag}_img"].to(gpu_device), gold[f"{tag}_enc"].to(gpu_device),
                   int(gold[f"{tag}_it"]), theta=gold[f"{tag}_theta"].to(gpu_device))
        assert float(loss) == pytest.approx(float(gold[f"{tag}_loss"]), rel=FWD_TOL)
        # the encoder saw the rotated batch
        gap = losses_ref.normwise(model.seen, gold[f"{tag}_img_rot"])
        assert (gap <= 2 * FWD_TOL).all(), gap.tolist()
        assert mod.diffs == []  # nothing is kept without a log
    for tag in ("cta", "ctb"):
        enc = gold[f"{tag}_enc"].to(gpu_device)
        num = EncoderContinuityLoss(None, lamb=0.7)
        assert float(num(enc, 5)) == pytest.approx(float(gold[f"{tag}_loss"]), rel=FWD_TOL)
        sched = EncoderContinuityLoss(None, lamb=_schedule)
        assert float(sched(enc, int(gold[f"{tag}_it"]))) == pytest.approx(
            float(gold[f"{tag}_loss_sched"]), rel=FWD_TOL)
        assert num.diffs == [] and sched.diffs == []


def test_equivariance_numeric_lamb_and_num_samples(gpu_device):
    """lamb as a plain number (the reference's own default 1.0 fails at self.lamb(it)) and
    num_samples: only the first images and encodings enter."""
    from lie_vae.losses import EquivarianceLoss
    gold = {k: torch.from_numpy(v) for k, v in golden("losses.npz").items()}
    k = 3
    model = _StubModel(gold["eqa_enc_rot"][:k].to(gpu_device))
    mod = EquivarianceLoss(model, num_samples=k, lamb=2.0)
    loss = mod(gold["eqa_img"].to(gpu_device), gold["eqa_enc"].to(gpu_device), 0,
               theta=gold["eqa_theta"][:k].to(gpu_device))
    assert model.seen.shape[0] == k
    assert float(loss) == pytest.approx(2.0 * float(gold["eqa_diffs"][:k].mean()), rel=FWD_TOL)
    # without theta the angles are drawn on the encoding's device
    torch.manual_seed(5)
    a = EquivarianceLoss(model, num_samples=k)(gold["eqa_img"].to(gpu_device),
                                               gold["eqa_enc"].to(gpu_device), 0)
    torch.manual_seed(5)
    theta = torch.rand(k, device=gpu_device) * 2 * math.pi
    b = EquivarianceLoss(model, num_samples=k)(gold["eqa_img"].to(gpu_device),
                                               gold["eqa_enc"].to(gpu_device), 0, theta=theta)
    assert torch.equal(a, b)


def test_modules_log_cadence(gpu_device):
    """Scalars go to the log whenever (it + 1) % report_freq == 0, at step it + 1, with the
    reference's tags: the mean of the diffs since the last report, then lamb
    (equivariance_loss.py:42-46, encoder_continuity_loss.py:29-33)."""
    from lie_vae.losses import EncoderContinuityLoss, EquivarianceLoss
    g = torch.Generator().manual_seed(9)
    img = torch.rand(4, 1, 16, 16, generator=g).to(gpu_device)
    enc = torch.randn(4, 3, 3, generator=g).to(gpu_device)
    model = _StubModel(torch.randn(4, 3, 3, generator=g).to(gpu_device))
    for make, tag in ((lambda log: EquivarianceLoss(model, lamb=_schedule, log=log, report_freq=3),
                       "equivariance"),
                      (lambda log: EncoderContinuityLoss(None, lamb=_schedule, log=log, report_freq=3),
                       "encoder_continuity")):
        log = _StubLog()
        mod = make(log)
        per_step = []
        for it in range(1, 9):  # the trainer's global_it counts from 1
            theta = torch.rand(4, generator=g).to(gpu_device) * 2 * math.pi
            loss = mod(img, enc, it, theta=theta) if tag == "equivariance" else mod(enc + it, it)
            per_step.append(float(loss) / _schedule(it))
        assert [c[0] for c in log.calls] == [tag, tag + "_lamb"] * 3
        assert [c[2] for c in log.calls] == [3, 3, 6, 6, 9, 9]
        assert [c[1] for c in log.calls[1::2]] == [_schedule(2), _schedule(5), _schedule(8)]
        # it = 1, 2 | 3, 4, 5 | 6, 7, 8: means of the steps since the last report
        want = [sum(per_step[0:2]) / 2, sum(per_step[2:5]) / 3, sum(per_step[5:8]) / 3]
        assert [c[1] for c in log.calls[0::2]] == pytest.approx(want, rel=1e-5)
        assert mod.diffs == []


# ---------------------------------------------------------------- trainer
@pytest.mark.parametrize("batch_norm", [False, True], ids=["convnet", "convnet_bn"])
def test_dp_trainer_step_with_regularisers(gpu_device, batch_norm):
    """One DPTrainer step with both terms on a toy-size conv VAE at batch 8: the encoder's
    gradients move away from the plain step's and match, to the gradient tolerance, a step
    whose extra terms are the torch ops of losses_ref on the device with the same angles (the
    device generator is reseeded, and both steps draw in the same order: theta, then the
    second pass's noise).

    The comparison is only as good as the reference step is reproducible.  Its rotation
    (affine_grid + grid_sample) and the kernel's each sit within ~1e-6 of fp64, and the second
    encoder pass amplifies such a difference.  Measured on the reference step alone, by adding
    a 1e-6 normwise perturbation to ITS rotated batch and differencing its own gradients: the
    plain ConvNet encoder changes by 5e-7, the BatchNorm encoder (batch statistics over 8
    images) by 7e-5 on these noise images and 1.1e-3 on smooth ones.  So with BatchNorm the
    torch-rotation reference does not determine the gradient to 1e-4 (the trainer's step
    differed from it by 7.5e-4, and by 2.5e-7 once that reference was given the same rotated
    batch).  Hence: the ConvNet model is held to the reference with torch's own rotation; the
    BatchNorm model to the reference with every other op from losses_ref and the rotated
    batch from rotate_images, which test_rotation_vs_fp64 holds to fp64."""
    import lie_vae._ops as ops
    from lie_vae.experiments.train_dp import DPTrainer
    from lie_vae.experiments.vae import VAE
    det, bench = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        torch.manual_seed(0)
        base = VAE(latent_mode="so3", decoder_mode="action", degrees=3, rep_copies=4, rgb=False,
                   batch_norm=batch_norm, deconv_hidden=8, mean_mode="alg").to(gpu_device)
        g = torch.Generator().manual_seed(2)
        x = torch.rand(8, 1, 64, 64, generator=g).to(gpu_device)
        eps = torch.randn(1, 8, 3, generator=g).to(gpu_device)
        lam_e, lam_c = 0.8, _schedule  # a number and a schedule
        rotate = ops.rotate_images if batch_norm else losses_ref.rotate

        def enc_grads(m):
            ps = list(m.encoder.parameters()) + list(m.rep_group.parameters())
            return torch.cat([p.grad.detach().flatten().double() for p in ps]).cpu()

        m_plain = copy.deepcopy(base)
        DPTrainer(m_plain, lr=1e-3, clip_grads=0).step(x, eps)
        g_plain = enc_grads(m_plain)

        m_reg = copy.deepcopy(base)
        tr = DPTrainer(m_reg, lr=1e-3, clip_grads=0, equivariance_lamb=lam_e,
                       encoder_continuity_lamb=lam_c)
        torch.manual_seed(77)
        loss_reg, _, _ = tr.step(x, eps)
        g_reg = enc_grads(m_reg)

        m_ref = copy.deepcopy(base)
        torch.manual_seed(77)
        recon, kl, _ = m_ref.elbo(x, n=1, eps=eps)
        loss = (recon + 1.0 * kl).mean()
        z = m_ref.z[0][0]
        theta = torch.rand(8, device=gpu_device) * 2 * math.pi
        cs = losses_ref.cos_sin(theta)
        z_rot = m_ref.encode(rotate(x, cs))[0][0]
        loss = loss + losses_ref.equivariance_diffs(cs, z, z_rot).mean() * lam_e
        loss = loss + losses_ref.pair_sqdist(z).mean() * lam_c(1)
        loss.backward()
        g_ref = enc_grads(m_ref)
        torch.cuda.synchronize()

        assert torch.isfinite(g_reg).all() and torch.isfinite(loss_reg)
        moved = float((g_reg - g_plain).norm() / g_plain.norm())
        err = float((g_reg - g_ref).norm() / g_ref.norm())
        print(f"trainer step (batch_norm={batch_norm}): regularisers move the encoder gradient "
              f"by {moved:.3e} (normwise); vs torch-op terms {err:.3e}; "
              f"loss {float(loss_reg):.6f} vs {float(loss.detach()):.6f}")
        assert moved > 100 * GRAD_TOL
        assert err <= GRAD_TOL
        assert float(loss_reg) == pytest.approx(float(loss.detach()), rel=FWD_TOL)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det, bench


# ---------------------------------------------------------------- graph
def test_rotate_and_diff_graph_replay_bitwise(gpu_device):
    """rotate_images + equivariance_diff captured on one stream and replayed give the eager
    results bit for bit (the calls are asynchronous on the caller's stream and allocate
    nothing themselves)."""
    import lie_vae._ops as ops
    g = torch.Generator().manual_seed(21)
    img = torch.rand(6, 3, 64, 64, generator=g).to(gpu_device)
    cs = losses_ref.cos_sin(torch.rand(6, generator=g) * 2 * math.pi).to(gpu_device)
    enc = torch.randn(6, 3, 3, generator=g).to(gpu_device)
    enc_rot = torch.randn(6, 3, 3, generator=g).to(gpu_device)

    def run():
        return ops.rotate_images(img, cs), ops.equivariance_diff(cs, enc, enc_rot)

    eager = [t.clone() for t in run()]
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    # new inputs in the static buffers, same graph
    img.copy_(img.flip(0))
    graph.replay()
    want = [t.clone() for t in run()]
    torch.cuda.synchronize()
    for a, b in zip(want, out):
        assert torch.equal(a, b)
