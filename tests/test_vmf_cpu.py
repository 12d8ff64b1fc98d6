"""CPU checks of the vMF latent on S^3 (csrc/vmf.hip, lie_vae.reparameterize.Sreparameterize):
the module's API against the reference's names, the six C entry points and their argument
checks (no device needed: the checks run before any launch), the refusal of CPU tensors, and
the fp64 restatement in tests/vmf_ref.py against independent facts: quadrature of the density,
finite differences, the geometry of the reflection, and the moments of 2·10^5 samples."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch
from scipy.integrate import quad

import vmf_ref
from conftest import REPO

ENTRY_POINTS = ("lv_vmf_sample_fwd", "lv_vmf_sample_bwd", "lv_vmf_kl_fwd", "lv_vmf_kl_bwd",
                "lv_vmf_log_prob_fwd", "lv_vmf_log_prob_bwd")
F64 = torch.float64


def test_sreparameterize_api_matches_reference_names():
    """Constructor, attributes and methods of reparameterize.py:58-97; the only additions are
    the trailing noise=None of forward / nsample and the `trials` attribute."""
    from lie_vae.reparameterize import Sreparameterize

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert params(Sreparameterize.__init__) == [("self", E), ("input_dim", E), ("z_dim", E)]
    assert params(Sreparameterize.forward) == [("self", E), ("x", E), ("n", 1), ("noise", None)]
    assert params(Sreparameterize.nsample) == [("self", E), ("n", 1), ("noise", None)]
    for name in ("kl", "log_posterior", "log_prior", "deterministic"):
        assert params(getattr(Sreparameterize, name)) == [("self", E)], name
    m = Sreparameterize(10, 4)
    assert isinstance(m, torch.nn.Module)
    assert (m.input_dim, m.z_dim, m.return_means, m.trials) == (10, 4, False, 16)
    assert m.mu is None and m.k is None and m.z is None
    assert tuple(m.k_linear.weight.shape) == (1, 10) and tuple(m.mu_linear.weight.shape) == (4, 10)
    m.deterministic()
    assert m.return_means is True
    for z_dim in (3, 5):
        with pytest.raises(NotImplementedError, match="S³"):
            Sreparameterize(10, z_dim)


def test_vae_builds_with_vmf_latents():
    from lie_vae.experiments.vae import VAE
    from lie_vae.reparameterize import Sreparameterize
    for mode, dec in (("vmf", "mlp"), ("vmfq", "action"), ("vmfq", "mlp")):
        vae = VAE(latent_mode=mode, decoder_mode=dec, degrees=3, deconv_mode="toy",
                  encode_mode="toy")
        assert isinstance(vae.rep_group, Sreparameterize)


def test_library_exports_the_vmf_entry_points():
    from lie_vae import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "lievae.h")).read()
    declared = set(re.findall(r"\b(lv_\w+)\s*\(", header))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
        assert name in declared, name
    assert lib.lv_abi_version() == 1


def test_argument_checks_before_any_launch():
    """Negative sizes, trials outside 1..64 and null pointers return LV_ERR_ARG with a message
    before anything is launched (dummy non-null pointers, no device); empty batches are LV_OK."""
    from lie_vae import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(16)  # never dereferenced: the checks run first

    def refused(rc, word):
        msg = lib.lv_last_error()
        assert rc == -1 and msg and word in msg, (rc, msg)

    sf, sb = lib.lv_vmf_sample_fwd, lib.lv_vmf_sample_bwd
    kf, kb = lib.lv_vmf_kl_fwd, lib.lv_vmf_kl_bwd
    lf, lb = lib.lv_vmf_log_prob_fwd, lib.lv_vmf_log_prob_bwd
    for ns, B in ((-1, 4), (4, -1), (-2, -2)):
        refused(sf(P, P, P, P, P, ns, B, 16, None), b"ns and B")
        refused(sb(P, P, P, P, P, P, P, ns, B, 16, None), b"ns and B")
        refused(lf(P, P, P, P, ns, B, None), b"ns and B")
        refused(lb(P, P, P, P, P, P, P, ns, B, None), b"ns and B")
    refused(kf(P, P, -1, None), b"B must")
    refused(kb(P, P, P, -1, None), b"B must")
    for trials in (0, 65, -1):
        refused(sf(P, P, P, P, P, 2, 3, trials, None), b"trials")
        refused(sb(P, P, P, P, P, P, P, 2, 3, trials, None), b"trials")
        refused(sf(P, P, P, P, P, 0, 3, trials, None), b"trials")  # also on an empty batch
    for i in range(5):
        a = [P] * 5
        a[i] = None
        refused(sf(*a, 2, 3, 16, None), b"null")
    for i in range(7):
        a = [P] * 7
        a[i] = None
        refused(sb(*a, 2, 3, 16, None), b"null")
        refused(lb(*a, 2, 3, None), b"null")
    for i in range(4):
        a = [P] * 4
        a[i] = None
        refused(lf(*a, 2, 3, None), b"null")
    refused(kf(None, P, 3, None), b"null")
    refused(kf(P, None, 3, None), b"null")
    for i in range(3):
        a = [P] * 3
        a[i] = None
        refused(kb(*a, 3, None), b"null")
    # empty batches: LV_OK, nothing launched (null pointers are then fine too)
    for ns, B in ((0, 5), (5, 0), (0, 0)):
        assert sf(P, P, P, P, P, ns, B, 16, None) == 0
        assert sf(None, None, None, None, None, ns, B, 1, None) == 0
        assert sb(P, P, P, P, P, P, P, ns, B, 64, None) == 0
        assert lf(P, P, P, P, ns, B, None) == 0
        assert lb(P, P, P, P, P, P, P, ns, B, None) == 0
    assert kf(P, P, 0, None) == 0 and kb(P, P, P, 0, None) == 0


def test_cpu_tensors_fail_loudly():
    import lie_vae._ops as ops
    from lie_vae.reparameterize import Sreparameterize
    mu = torch.nn.functional.normalize(torch.randn(3, 4), dim=-1)
    kappa = torch.rand(3) + 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vmf_sample(mu, kappa, torch.randn(2, 3, 99))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vmf_kl(kappa)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vmf_log_prob(mu, kappa, mu.expand(2, -1, -1))
    m = Sreparameterize(10, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(3, 10), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(3, 10), 2, noise=torch.randn(2, 3, 99))


def test_ops_shape_asserts():
    import lie_vae._ops as ops
    mu, kappa = torch.randn(3, 4), torch.rand(3) + 1
    with pytest.raises(AssertionError, match="noise width"):
        ops.vmf_sample(mu, kappa, torch.randn(2, 3, 98))
    with pytest.raises(AssertionError, match="noise width"):
        ops.vmf_sample(mu, kappa, torch.randn(2, 3, 6 * 65 + 3))
    with pytest.raises(AssertionError, match="mu must"):
        ops.vmf_sample(mu[:2], kappa, torch.randn(2, 3, 99))
    with pytest.raises(AssertionError, match="kappa must"):
        ops.vmf_sample(mu, kappa[:, None], torch.randn(2, 3, 99))
    with pytest.raises(AssertionError, match="z must"):
        ops.vmf_log_prob(mu, kappa, torch.randn(2, 3, 3))
    with pytest.raises(AssertionError, match="kappa must"):
        ops.vmf_kl(kappa[:, None])


# ------------------------------------------------------------ restatement vs facts
def _quad_moments(kappa):
    """ln C + kappa and E[mu.z] by quadrature of the density over w = mu.z = 1 - s^2: the
    measure on S^3 is 4 pi sqrt(1 - w^2) dw, so the scaled normaliser is
    int exp(-kappa s^2) 4 pi s sqrt(2 - s^2) 2 s ds, smooth in s on [0, sqrt 2]."""
    def dens(s):
        return math.exp(-kappa * s * s) * 8 * math.pi * s * s * math.sqrt(2 - s * s)
    width = min(math.sqrt(2), 12 / math.sqrt(kappa))
    pts = dict(epsabs=0, epsrel=1e-13, limit=400)
    Z = quad(dens, 0, width, **pts)[0]
    if width < math.sqrt(2):
        Z += quad(dens, width, math.sqrt(2), **pts)[0]
    Ew1 = quad(lambda s: s * s * dens(s), 0, width, **pts)[0]  # E[1 - w] Z
    if width < math.sqrt(2):
        Ew1 += quad(lambda s: s * s * dens(s), width, math.sqrt(2), **pts)[0]
    return -math.log(Z), 1 - Ew1 / Z, Ew1 / Z


@pytest.mark.parametrize("kappa", [1.0, 3.0, 30.0, 300.0])
def test_kl_against_quadrature(kappa):
    """KL = E[ln q] + ln(2 pi^2) = (ln C + kappa) - kappa E[1 - w] + ln(2 pi^2), every piece
    from quadrature; 1e-9 relative."""
    lnck, A, one_minus_A = _quad_moments(kappa)
    want = lnck - kappa * one_minus_A + vmf_ref.LOG_AREA_S3
    k = torch.tensor([kappa], dtype=F64)
    got = float(vmf_ref.kl(k))
    print(f"kappa={kappa}: KL {got:.12f} quad {want:.12f} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-9 * abs(want)
    assert abs(float(vmf_ref.ratio(k)) - A) <= 1e-9 * A
    assert abs(float(vmf_ref.log_norm_shifted(k)) - lnck) <= 1e-9 * abs(lnck)
    # dKL/dkappa = kappa A' by central differences of the quadrature-checked KL
    h = 1e-4 * kappa
    fd = (float(vmf_ref.kl(k + h)) - float(vmf_ref.kl(k - h))) / (2 * h)
    assert abs(float(vmf_ref.dkl_dkappa(k)) - fd) <= 1e-6 * abs(fd)


def test_gradcheck_kl_log_prob_and_sample():
    gen = torch.Generator().manual_seed(5)
    kappa = torch.tensor([1.0, 3.0, 19.5, 30.0, 300.0], dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(vmf_ref.kl, (kappa,))
    assert torch.autograd.gradcheck(vmf_ref.log_norm_shifted, (kappa,))
    B, ns, T = 5, 3, 16
    # means away from mu[0] = 0, where the reflection changes branch (both signs present)
    mu = torch.randn(B, 4, generator=gen, dtype=F64)
    mu = (mu / mu.norm(dim=-1, keepdim=True)).requires_grad_(True)
    assert (mu[:, 0].abs() > 1e-2).all() and (mu[:, 0] > 0).any() and (mu[:, 0] < 0).any()
    noise = torch.randn(ns, B, 6 * T + 3, generator=gen, dtype=F64)
    with torch.no_grad():
        z0, acc, _ = vmf_ref.sample(mu, kappa, noise)
    assert torch.autograd.gradcheck(lambda m, k: vmf_ref.sample(m, k, noise, acc)[0], (mu, kappa))
    z = z0.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(vmf_ref.log_prob, (mu, kappa, z))
    # the closed forms of the issue: db/dkappa = -2b/c and dw/db = -2 eps (1 - eps) / D^2
    k = kappa.detach().clone().requires_grad_(True)
    _, b, c, _ = vmf_ref.constants(k)
    (db,) = torch.autograd.grad(b.sum(), k)
    assert torch.allclose(db, (-2 * b / c).detach(), rtol=1e-12, atol=0)
    # d = 4ab/(1+b) - 3 ln 3 is the constant 3 - 3 ln 3 (ab = 3 (1 + b) / 4)
    a, b, _, d = vmf_ref.constants(kappa.detach())
    assert torch.allclose(d, torch.full_like(d, 3 - 3 * math.log(3.0)), rtol=0, atol=1e-14)


def test_samples_are_unit_and_reflection_takes_e1_to_mu():
    gen = torch.Generator().manual_seed(6)
    B, ns, T = 64, 4, 16
    mu = vmf_ref.haar_mu(B, gen).double()
    mu = mu / mu.norm(dim=-1, keepdim=True)  # unit to fp64 for the exact statements below
    assert (mu[:, 0] <= 0).any() and (mu[:, 0] > 0).any()  # both branches
    e1 = torch.zeros(B, 4, dtype=F64)
    e1[:, 0] = 1
    assert (vmf_ref.reflect(mu, e1) - mu).abs().max() <= 1e-15
    # orthogonal: norms and inner products are kept
    x, y = torch.randn(2, B, 4, generator=gen, dtype=F64)
    qx, qy = vmf_ref.reflect(mu, x), vmf_ref.reflect(mu, y)
    assert ((qx * qy).sum(-1) - (x * y).sum(-1)).abs().max() <= 1e-13
    kappa = vmf_ref.cycle_kappa(B).double()
    noise = torch.randn(ns, B, 6 * T + 3, generator=gen, dtype=F64)
    z, acc, margin = vmf_ref.sample(mu, kappa, noise)
    assert (z.norm(dim=-1) - 1).abs().max() <= 1e-14
    assert acc.max() < T and acc.min() == 0
    # the accepted trial is the first with a non-negative margin
    first = margin.gather(-1, acc[..., None])[..., 0]
    assert (first >= 0).all()
    earlier = torch.arange(T) < acc[..., None]
    assert (margin[earlier] < 0).all()


def test_fallback_uses_the_last_proposal():
    """With one trial the restatement reports 1 where the trial is rejected and still returns
    that proposal's point."""
    gen = torch.Generator().manual_seed(7)
    B, ns = 40, 8
    mu, kappa = vmf_ref.haar_mu(B, gen).double(), vmf_ref.cycle_kappa(B).double()
    noise = torch.randn(ns, B, 9, generator=gen, dtype=F64)
    z, acc, margin = vmf_ref.sample(mu, kappa, noise)
    assert torch.equal(acc, (margin[..., 0] < 0).long())
    assert 0 < int(acc.sum()) < acc.numel()
    forced, _, _ = vmf_ref.sample(mu, kappa, noise, torch.zeros_like(acc))
    assert torch.equal(z, forced)


@pytest.mark.parametrize("kappa", [1.0, 30.0, 1e3, 1e5])
def test_sample_moments(kappa):
    """2·10^5 samples: the mean of mu.z within 5 standard errors of A(kappa), the standard
    error from the variance A'(kappa); the sample variance within 5 % of A' (its own standard
    error is sqrt((kurtosis - 1) / N) <= 0.6 % here: the kurtosis is at most 7, that of the
    chi^2_3 limit at large kappa); no sample exhausts 16 trials.  1 - mu.z is formed as
    |z - mu|^2 / 2 so that kappa = 1e5 keeps its digits."""
    N, T = 200_000, 16
    gen = torch.Generator().manual_seed(int(kappa) + 11)
    mu = torch.tensor([[0.5, -0.5, 0.5, 0.5]], dtype=F64)
    k = torch.tensor([kappa], dtype=F64)
    A, var = float(vmf_ref.ratio(k)), float(vmf_ref.ratio_prime(k))
    omw, longest = [], 0
    for _ in range(4):
        noise = torch.randn(N // 4, 1, 6 * T + 3, generator=gen, dtype=F64)
        z, acc, _ = vmf_ref.sample(mu, k, noise)
        longest = max(longest, int(acc.max()) + 1)
        omw.append(((z - mu) ** 2).sum(-1).flatten() / 2)
    omw = torch.cat(omw)
    se = math.sqrt(var / N)
    mean_err = abs(float(omw.mean()) - (1 - A))
    print(f"kappa={kappa}: mean(mu.z) - A = {mean_err:.3e} ({mean_err / se:.2f} s.e.), "
          f"var / A' = {float(omw.var()) / var:.4f}, longest run {longest} trials")
    assert longest <= T
    assert mean_err <= 5 * se
    assert abs(float(omw.var()) / var - 1) <= 0.05


def test_parity_seeds_stay_within_the_exclusion_cap():
    """The GPU parity test leaves out a sample whose acceptance margin is within 1e-4 of zero
    in some trial it reaches; with the committed seeds that is at most 1e-3 of the samples (none
    in the small cases), and every special mean row is present."""
    total = excluded = 0
    for ns, B in vmf_ref.PARITY_SHAPES:
        case = vmf_ref.parity_case(ns, B)
        n_close = int(case["close"].sum())
        print(f"(ns, B) = ({ns}, {B}): {n_close} of {ns * B} samples within "
              f"{vmf_ref.MARGIN_EXCLUDE} of the acceptance boundary; longest run "
              f"{int(case['accepted'].max()) + 1}")
        assert n_close <= vmf_ref.MAX_EXCLUDED * ns * B
        assert int(case["accepted"].max()) < 16
        total, excluded = total + ns * B, excluded + n_close
    assert excluded <= vmf_ref.MAX_EXCLUDED * total
    mu = vmf_ref.parity_case(4, 2048)["mu"]
    assert mu[0, 0] == 1 and mu[1, 0] == -1 and mu[2, 0] == 0
    assert 0 < (mu[3] - mu[0]).norm() < 1e-4
    assert sorted(set(vmf_ref.parity_case(3, 67)["kappa"].tolist())) == sorted(vmf_ref.KAPPAS)
