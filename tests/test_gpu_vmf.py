"""GPU tests of the vMF latent on S^3 (csrc/vmf.hip through lie_vae._ops and
lie_vae.reparameterize.Sreparameterize) against the fp64 restatement in tests/vmf_ref.py on
the same injected noise: the sampler and its accepted indices, the pathwise gradients, KL and
log-density with their gradients on both sides of the Bessel series crossover, the one-trial
fallback, moments of device-drawn samples, determinism, the module, the VAE's vmf / vmfq modes,
and graph replay.

Tolerances are DESIGN.md §2's: forward 1e-5 and gradients 1e-4, normwise.  A gradient that is
a sum of per-sample terms which may cancel (gkappa, a scalar per datum) is held to 1e-4 of
the sum of the terms' magnitudes."""
import pytest
import torch

import vmf_ref

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-5, 1e-4
F64 = torch.float64
# both sides of the ascending / asymptotic series crossover at kappa = 20
KL_KAPPAS = (1.0, 1.0 + 1e-3, 5.0, 19.0, 20.0, 21.0, 100.0, 1e3, 1e5)


def _gz(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------- sampler
@pytest.mark.parametrize("ns,B", vmf_ref.PARITY_SHAPES)
def test_sampler_matches_restatement_on_injected_noise(gpu_device, ns, B):
    """Same accepted trial and z within FWD_TOL for every sample except those the restatement
    itself flags (|margin| < 1e-4 in a trial it reaches: fp32 may decide it the other way), at
    most 1e-3 of the samples."""
    import lie_vae._ops as ops
    case = vmf_ref.parity_case(ns, B)
    z = ops.vmf_sample(case["mu"].to(gpu_device), case["kappa"].to(gpu_device),
                       case["noise"].to(gpu_device))
    acc = ops.vmf_last_accepted()
    assert z.shape == (ns, B, 4) and z.dtype == torch.float32
    assert acc.shape == (ns, B) and acc.dtype == torch.int32 and not acc.requires_grad
    z, acc = z.cpu(), acc.cpu().long()
    keep = ~case["close"]
    left_out = int(case["close"].sum())
    assert left_out <= vmf_ref.MAX_EXCLUDED * ns * B
    err = vmf_ref.normwise(z, case["z"])
    differ = int((acc != case["accepted"]).sum())
    print(f"(ns, B) = ({ns}, {B}): {left_out} left out, {differ} accepted indices differ in all, "
          f"max normwise err {float(err[keep].max()):.3e}, "
          f"| |z| - 1 | max {float((z.double().norm(dim=-1) - 1).abs().max()):.3e}")
    assert torch.equal(acc[keep], case["accepted"][keep])
    assert (err[keep] <= FWD_TOL).all()
    assert ((z.double().norm(dim=-1) - 1).abs() <= 1e-6).all()


@pytest.mark.parametrize("ns,B", vmf_ref.PARITY_SHAPES)
def test_sampler_gradients_match_fp64_autograd(gpu_device, ns, B):
    """gmu and gkappa of lv_vmf_sample_bwd against fp64 autograd of the restatement on the
    same noise and the kernel's own (frozen) accepted indices."""
    import lie_vae._ops as ops
    case = vmf_ref.parity_case(ns, B)
    mu = case["mu"].to(gpu_device).requires_grad_(True)
    kappa = case["kappa"].to(gpu_device).requires_grad_(True)
    gz = _gz((ns, B, 4), 31 + B)
    z = ops.vmf_sample(mu, kappa, case["noise"].to(gpu_device))
    acc = ops.vmf_last_accepted().cpu().long()
    z.backward(gz.to(gpu_device))
    gmu, gk, _, terms = vmf_ref.sample_grads(case["mu"].double(), case["kappa"].double(),
                                             case["noise"].double(), acc, gz.double())
    err_mu = vmf_ref.normwise(mu.grad.cpu(), gmu)
    scale = terms.abs().sum(0)
    err_k = (kappa.grad.cpu().double() - gk).abs() / scale
    print(f"(ns, B) = ({ns}, {B}): gmu normwise max {float(err_mu.max()):.3e}, "
          f"gkappa / sum|terms| max {float(err_k.max()):.3e}")
    assert (err_mu <= GRAD_TOL).all()
    assert (err_k <= GRAD_TOL).all()


def test_one_trial_falls_back_to_its_proposal(gpu_device):
    """trials = 1: accepted == 1 exactly where the restatement rejects the only trial, and z is
    that proposal's point either way."""
    import lie_vae._ops as ops
    ns, B = 8, 40
    case = vmf_ref.parity_case(ns, B, 1)
    assert not case["close"].any()  # no margin near zero with this seed: the comparison is exact
    assert case["noise"].shape[-1] == 9
    z = ops.vmf_sample(case["mu"].to(gpu_device), case["kappa"].to(gpu_device),
                       case["noise"].to(gpu_device)).cpu()
    acc = ops.vmf_last_accepted().cpu().long()
    rejected = (case["margin"][..., 0] < 0).long()
    assert 0 < int(rejected.sum()) < ns * B
    assert torch.equal(acc, rejected)
    forced, _, _ = vmf_ref.sample(case["mu"].double(), case["kappa"].double(),
                                  case["noise"].double(), torch.zeros_like(acc))
    assert (vmf_ref.normwise(z, forced) <= FWD_TOL).all()


@pytest.mark.parametrize("kappa", [1.0, 30.0, 1e3])
def test_device_drawn_samples_have_the_vmf_moments(gpu_device, kappa):
    """65,536 samples from torch.randn on the device: on the sphere to 1e-6, the mean of mu.z
    within 5 standard errors of A(kappa) (variance A'(kappa)), at most 6 samples exhausted."""
    import lie_vae._ops as ops
    N, T = 65536, 16
    torch.manual_seed(1234 + int(kappa))
    noise = torch.randn(N, 1, 6 * T + 3, device=gpu_device)
    mu = torch.tensor([[0.5, -0.5, 0.5, 0.5]], device=gpu_device)
    z = ops.vmf_sample(mu, torch.tensor([kappa], device=gpu_device), noise)
    acc = ops.vmf_last_accepted()
    k = torch.tensor([kappa], dtype=F64)
    A, var = float(vmf_ref.ratio(k)), float(vmf_ref.ratio_prime(k))
    omw = ((z.double() - mu.double()) ** 2).sum(-1).flatten() / 2  # 1 - mu.z on the sphere
    off = float((z.double().norm(dim=-1) - 1).abs().max())
    se = (var / N) ** 0.5
    mean_err = abs(float(omw.mean()) - (1 - A))
    exhausted = int((acc == T).sum())
    print(f"kappa={kappa}: | |z| - 1 | max {off:.3e}, mean(mu.z) - A = {mean_err:.3e} "
          f"({mean_err / se:.2f} s.e.), exhausted {exhausted}, longest run {int(acc.max()) + 1}")
    assert off <= 1e-6
    assert mean_err <= 5 * se
    assert exhausted <= 6
    assert int(acc.min()) == 0 and int(acc.max()) <= T


def test_backward_is_bitwise_reproducible(gpu_device):
    import lie_vae._ops as ops
    case = vmf_ref.parity_case(4, 2048)
    noise = case["noise"].to(gpu_device)
    gz = _gz((4, 2048, 4), 77).to(gpu_device)
    gout = _gz((4, 2048), 78).to(gpu_device)
    runs = []
    for _ in range(2):
        mu = case["mu"].to(gpu_device).requires_grad_(True)
        kappa = case["kappa"].to(gpu_device).requires_grad_(True)
        z = ops.vmf_sample(mu, kappa, noise)
        lp = ops.vmf_log_prob(mu, kappa, z)
        torch.autograd.backward([z, lp], [gz, gout])
        runs.append((mu.grad.clone(), kappa.grad.clone(), z.detach().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- KL and log-density
def test_kl_and_its_gradient(gpu_device):
    import lie_vae._ops as ops
    kap32 = torch.tensor(KL_KAPPAS, dtype=torch.float32)
    kappa = kap32.to(gpu_device).requires_grad_(True)
    kl = ops.vmf_kl(kappa)
    g = torch.linspace(0.5, 1.5, len(KL_KAPPAS))
    kl.backward(g.to(gpu_device))
    want = vmf_ref.kl(kap32.double())
    gwant = g.double() * vmf_ref.dkl_dkappa(kap32.double())
    err = (kl.detach().cpu().double() - want).abs() / want.abs()
    gerr = (kappa.grad.cpu().double() - gwant).abs() / gwant.abs()
    print(f"KL rel err max {float(err.max()):.3e}; dKL/dkappa rel err max {float(gerr.max()):.3e}")
    assert kl.shape == (len(KL_KAPPAS),)
    assert (err <= FWD_TOL).all(), err.tolist()
    assert (gerr <= GRAD_TOL).all(), gerr.tolist()


def test_log_prob_and_its_gradients(gpu_device):
    """z drawn by the restatement at each kappa (so near the mode at large kappa, where the
    subtracting form kappa (mu.z) would lose digits), then rounded to fp32."""
    import lie_vae._ops as ops
    gen = torch.Generator().manual_seed(91)
    B, ns, T = len(KL_KAPPAS), 5, 16
    mu32 = vmf_ref.haar_mu(B, gen)
    kap32 = torch.tensor(KL_KAPPAS, dtype=torch.float32)
    noise = torch.randn(ns, B, 6 * T + 3, generator=gen, dtype=F64)
    z32 = vmf_ref.sample(mu32.double(), kap32.double(), noise)[0].float()
    gout = _gz((ns, B), 92)
    mu = mu32.to(gpu_device).requires_grad_(True)
    kappa = kap32.to(gpu_device).requires_grad_(True)
    z = z32.to(gpu_device).requires_grad_(True)
    out = ops.vmf_log_prob(mu, kappa, z)
    out.backward(gout.to(gpu_device))
    want = vmf_ref.log_prob(mu32.double(), kap32.double(), z32.double())
    gmu, gk, gz, _, kterms = vmf_ref.log_prob_grads(mu32.double(), kap32.double(), z32.double(),
                                                    gout.double())
    err = vmf_ref.normwise(out.detach().cpu().T, want.T)  # per datum, over its samples
    err_mu = vmf_ref.normwise(mu.grad.cpu(), gmu)
    err_z = vmf_ref.normwise(z.grad.cpu(), gz)
    err_k = (kappa.grad.cpu().double() - gk).abs() / kterms.abs().sum(0)
    print(f"log q normwise max {float(err.max()):.3e}; gmu {float(err_mu.max()):.3e}, "
          f"gz {float(err_z.max()):.3e}, gkappa / sum|terms| {float(err_k.max()):.3e}")
    assert out.shape == (ns, B)
    assert (err <= FWD_TOL).all(), err.tolist()
    assert (err_mu <= GRAD_TOL).all() and (err_z <= GRAD_TOL).all(), (err_mu, err_z)
    assert (err_k <= GRAD_TOL).all(), err_k.tolist()


# ---------------------------------------------------------------- module and VAE
def test_module_shapes_values_and_deterministic(gpu_device):
    import math

    from lie_vae.reparameterize import Sreparameterize
    torch.manual_seed(3)
    m = Sreparameterize(10, 4).to(gpu_device)
    x = torch.randn(7, 10, device=gpu_device)
    z = m(x, 3)
    assert z.shape == (3, 7, 4) and m.mu.shape == (7, 4) and m.k.shape == (7, 1)
    assert m.kl().shape == (7,)
    assert m.log_posterior().shape == (3, 7) and m.log_prior().shape == (3, 7)
    assert (m.k >= 1).all()
    assert torch.allclose(m.log_prior(), torch.full((3, 7), -math.log(2 * math.pi ** 2),
                                                    device=gpu_device))
    # injected noise: the module's values are the restatement's on its own mu and k
    noise = torch.randn(3, 7, 6 * m.trials + 3, device=gpu_device)
    z = m(x, 3, noise=noise)
    mu64, k64 = m.mu.detach().cpu().double(), m.k.detach().cpu().double().reshape(-1)
    zr, acc, margin = vmf_ref.sample(mu64, k64, noise.cpu().double())
    upto = torch.arange(m.trials) <= acc.clamp(max=m.trials - 1)[..., None]
    keep = ~((margin.abs() < vmf_ref.MARGIN_EXCLUDE) & upto).any(-1)
    assert int(keep.sum()) >= keep.numel() - 1
    assert (vmf_ref.normwise(z.detach().cpu(), zr)[keep] <= FWD_TOL).all()
    assert ((m.kl().detach().cpu().double() - vmf_ref.kl(k64)).abs() <= FWD_TOL * vmf_ref.kl(k64)).all()
    lp = vmf_ref.log_prob(mu64, k64, z.detach().cpu().double())
    assert (vmf_ref.normwise(m.log_posterior().detach().cpu().T, lp.T) <= FWD_TOL).all()
    m.deterministic()
    z = m(x, 3)
    assert z.shape == (3, 7, 4) and torch.equal(z, m.mu.expand(3, -1, -1))
    assert m.log_posterior().shape == (3, 7)


@pytest.mark.parametrize("latent,decoder", [("vmfq", "action"), ("vmf", "mlp")])
def test_vae_elbo_backward_and_log_likelihood(gpu_device, latent, decoder):
    from lie_vae.experiments.vae import VAE
    torch.manual_seed(4)
    vae = VAE(latent_mode=latent, decoder_mode=decoder, degrees=3, deconv_mode="toy",
              encode_mode="toy").to(gpu_device)
    x = torch.randn(6, 16, 10, device=gpu_device)
    recon, kl, kls = vae.elbo(x, n=2)
    assert recon.shape == (2, 6) and kl.shape == (6,) and len(kls) == 1
    (recon + kl).mean().backward()
    for name, p in vae.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert any(float(p.grad.abs().max()) > 0 for p in vae.rep_group.parameters())
    # injected noise travels through encode's eps
    noise = torch.randn(2, 6, 6 * vae.rep_group.trials + 3, device=gpu_device)
    a = vae.elbo(x, n=2, eps=noise)[0]
    b = vae.elbo(x, n=2, eps=noise)[0]
    assert torch.equal(a, b)
    ll = vae.log_likelihood(x, n=5)
    assert ll.dim() == 0 and torch.isfinite(ll)


# ---------------------------------------------------------------- graph
def test_module_forward_backward_graph_replay_bitwise(gpu_device):
    """Forward + backward of the module on static noise, captured and replayed, give the eager
    results bit for bit and follow new noise written into the same buffer: one bounded launch
    per op, no host sync."""
    from lie_vae.reparameterize import Sreparameterize
    torch.manual_seed(8)
    m = Sreparameterize(10, 4).to(gpu_device)
    params = list(m.parameters())
    x = torch.randn(33, 10, device=gpu_device)
    noise = torch.randn(3, 33, 6 * m.trials + 3, device=gpu_device)
    wz = torch.randn(3, 33, 4, device=gpu_device)
    wl = torch.randn(3, 33, device=gpu_device)

    def run():
        """One step; the gradients land in fresh .grad tensors.  Nothing of the step's autograd
        graph is left alive afterwards (the module keeps its last mu / k / z, whose graph would
        hold the parameters' gradient accumulators and with them the stream they were made
        on: a later step on another stream, the capture's, would then reach across streams,
        which is what DPTrainer._drop_autograd_refs is for)."""
        for p in params:
            p.grad = None
        z = m(x, 3, noise=noise)
        lp = m.log_posterior()
        loss = (z * wz).sum() + m.kl().sum() + (lp * wl).sum() - m.log_prior().sum()
        loss.backward()
        m.mu = m.k = m.z = None
        return (z.detach(), lp.detach(), *[p.grad for p in params])

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
    # new noise in the static buffer, same graph
    noise.copy_(torch.randn_like(noise))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    want = run()
    for a, b in zip(want, replayed):
        assert torch.equal(a, b)
    assert not torch.equal(want[0], eager[0])
