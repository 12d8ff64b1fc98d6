"""GPU checks of the SO(3) projection family (csrc/so3_stats.hip; lie_tools.project_to_so3 /
so3_mean / align_rotations; reparameterize.SVDMean; experiments/pose_eval.py) against the
restatement in tests/so3_project_ref.py, which tests/test_so3_project_cpu.py pins to numpy's SVD,
autograd through torch.linalg.svd and central differences.

Per-sample bounds: err * gamma / eps <= 4 x the restatement's own constant on the same family
(gamma = (s2 + s3')/s1 from the fp64 SVD; 4x: the margin of a kernel whose operation order may
differ from its restatement), forward and backward, fp32 (eps = 2^-24) and fp64 (2^-53);
|R^T R - I| and |det R - 1| to 2x the restatement's worst, independently of gamma."""
import math

import pytest
import torch

import so3_project_ref as ref
from so3_log_ref import haar

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SIZES = (1, 255, 257, ref.FAMILY_N)      # one thread, the block edge, a block and a tail, 17 blocks
C_FWD = 22.4                             # the restatement's worst family (test_so3_project_cpu prints it)
FWD_BOUND_RAD = 4 * C_FWD * 2.0 ** -24


def host(t):
    return t.detach().cpu()


# ------------------------------------------------------------------ projection
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ref.FAMILIES)
def test_project_forward_backward(gpu_device, name, dtype):
    import lie_vae.lie_tools as lt
    c = ref.family_case(name, dtype)
    eps = ref.EPS[dtype]
    M = c["M"].to(gpu_device).requires_grad_(True)
    R = lt.project_to_so3(M)
    (gM,) = torch.autograd.grad(R, M, c["gR"].to(gpu_device))
    R, gM = host(R), host(gM)
    assert R.dtype == dtype and gM.dtype == dtype and R.shape == (ref.FAMILY_N, 3, 3)
    assert torch.isfinite(R).all() and torch.isfinite(gM).all()
    e_f = (R.double() - c["R64"]).flatten(1).norm(dim=-1) * c["gamma"] / eps
    e_b = ref.rel_err(gM, c["gM64"]) * c["gamma"] / eps
    eye = torch.eye(3, dtype=F64)
    orth = ((R.double().transpose(-1, -2) @ R.double()) - eye).flatten(1).norm(dim=-1).max().item()
    det = (torch.det(R.double()) - 1).abs().max().item()
    print(f"{name} {dtype}: fwd {float(e_f.max()):.1f} (restatement {c['c_fwd']:.1f}), "
          f"bwd {float(e_b.max()):.1f} ({c['c_bwd']:.1f}), orth {orth:.2e} ({c['orth']:.2e}), "
          f"det {det:.2e} ({c['det']:.2e})")
    assert (e_f <= 4 * c["c_fwd"]).all()
    assert (e_b <= 4 * c["c_bwd"]).all()
    assert orth <= 2 * c["orth"] and det <= 2 * c["det"]
    assert (torch.det(R.double()) > 0).all()
    # per-sample map: every size gives the bits of the same rows (ragged tails, one thread)
    for n in SIZES[:-1]:
        Mn = c["M"][:n].to(gpu_device).requires_grad_(True)
        Rn = lt.project_to_so3(Mn)
        (gn,) = torch.autograd.grad(Rn, Mn, c["gR"][:n].to(gpu_device))
        assert torch.equal(host(Rn), R[:n]) and torch.equal(host(gn), gM[:n]), n


def test_project_shapes_and_empty(gpu_device):
    import lie_vae.lie_tools as lt
    M = ref.family("noise_0.1")[:24].float().to(gpu_device)
    R = lt.project_to_so3(M)
    assert torch.equal(lt.project_to_so3(M.reshape(2, 3, 4, 3, 3)), R.reshape(2, 3, 4, 3, 3))
    assert torch.equal(lt.project_to_so3(M[5]), R[5])
    assert lt.project_to_so3(M[:0]).shape == (0, 3, 3)
    e = M[:0].clone().requires_grad_(True)
    lt.project_to_so3(e).sum().backward()
    assert e.grad.shape == (0, 3, 3)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_singular_set(gpu_device, dtype):
    """Zero, rank 1, diag(1, 1, -1), gamma = 2^-13 and its neighbour at 2^-11: the output is a
    rotation; the gradient is exactly 0 where gamma <= sqrt(eps) and non-zero beside it."""
    import lie_vae.lie_tools as lt
    S = ref.singular_set(dtype).to(gpu_device).requires_grad_(True)
    R = lt.project_to_so3(S)
    g = (torch.ones(5, 3, 3, dtype=dtype) * torch.arange(1, 10, dtype=dtype).reshape(3, 3)).to(gpu_device)
    (gM,) = torch.autograd.grad(R, S, g)
    R, gM = host(R).double(), host(gM)
    tol = 64 * ref.EPS[dtype]
    assert torch.isfinite(R).all() and torch.isfinite(gM).all()
    assert ((R.transpose(-1, -2) @ R - torch.eye(3, dtype=F64)).flatten(1).norm(dim=-1) <= tol).all()
    assert ((torch.det(R) - 1).abs() <= tol).all()
    assert torch.equal(R[0], torch.eye(3, dtype=F64))
    assert torch.equal(gM[:3], torch.zeros(3, 3, 3, dtype=dtype))
    if dtype == F32:
        assert torch.equal(gM[3], torch.zeros(3, 3)) and gM[4].abs().max() > 0
    else:
        assert gM[3].abs().max() > 0 and gM[4].abs().max() > 0


# ------------------------------------------------------------------ moment
@pytest.fixture(scope="module")
def moment_inputs():
    gen = torch.Generator().manual_seed(8400)
    n = 100003
    X, Y = haar(n, gen, F32), haar(n, gen, F32)
    w = (torch.rand(n, generator=gen, dtype=F64) + 0.1).float()
    C = haar(4, gen, F32)
    return X, Y, w, C


@pytest.mark.parametrize("n", [1, 4099, 100003])
@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
def test_moment_against_fp64_einsum_and_bitwise_repeatable(gpu_device, moment_inputs, n, weighted):
    """One thread, several blocks, several strides per thread; ns = 1 without C and ns = 4 with
    every transpose flag.  The fp32 inputs are exact in fp64, so only the summation order
    differs from the host's einsum: 1e-12 of sum w.  Two runs give equal bits."""
    import lie_vae._ops as ops
    from lie_vae import _lib
    X, Y, w, C = (t[:n] if t.shape[0] > 4 else t for t in moment_inputs)
    w = w if weighted else None
    wd = w.double() if weighted else torch.ones(n, dtype=F64)
    Xd, Yd, Cd = X.double(), Y.double(), C.double()
    dev = [None if t is None else t.to(gpu_device) for t in (X, Y, w, C)]
    cases = [((dev[0], None, dev[2], None, 0), torch.einsum("i,iab->ab", wd, Xd)[None]),
             ((dev[0], dev[1], dev[2], None, _lib.LV_MOMENT_YT),
              torch.einsum("i,iab,icb->ac", wd, Xd, Yd)[None]),
             ((dev[0], dev[1], dev[2], dev[3], 0), torch.einsum("i,iab,sbc,icd->sad", wd, Xd, Cd, Yd)),
             ((dev[0], dev[1], dev[2], dev[3], _lib.LV_MOMENT_XT | _lib.LV_MOMENT_YT | _lib.LV_MOMENT_CT),
              torch.einsum("i,iba,scb,idc->sad", wd, Xd, Cd, Yd))]
    for args, want in cases:
        S, ws, R = ops.so3_moment(*args)
        S2, ws2, R2 = ops.so3_moment(*args)
        assert S.dtype == F64 and ws.dtype == F64 and R.dtype == F32
        assert torch.equal(S, S2) and torch.equal(ws, ws2) and torch.equal(R, R2)
        S, ws, R = host(S), host(ws), host(R)
        err = (S - want).abs().max().item() / wd.sum().item()
        print(f"n={n} flags={args[4]} ns={want.shape[0]}: |S - einsum| / sum w = {err:.2e}")
        assert err <= 1e-12
        assert abs(ws.item() - wd.sum().item()) <= 1e-12 * wd.sum().item()
        # R = the fp64 projection of that S, rounded to the input type
        R64, gamma = ref.svd_project(S), ref.svd_gamma(S)
        assert ((R.double() - R64).flatten(1).norm(dim=-1) * gamma <= 4 * 2.0 ** -24).all()
    # the fp64 twin on the same values
    S64, _, R64 = ops.so3_moment(dev[0].double(), dev[1].double(), None if w is None else dev[2].double(),
                                 dev[3].double(), cases[2][0][4])
    assert R64.dtype == F64
    assert (host(S64) - cases[2][1]).abs().max().item() <= 1e-12 * wd.sum().item()
    assert ((host(R64) - ref.svd_project(host(S64))).flatten(1).norm(dim=-1) * ref.svd_gamma(host(S64))
            <= 1e-12).all()


def test_moment_of_the_empty_set_and_mean(gpu_device):
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    e = torch.zeros(0, 3, 3, device=gpu_device)
    S, ws, R = ops.so3_moment(e)
    assert torch.equal(host(S), torch.zeros(1, 3, 3, dtype=F64)) and ws.item() == 0.0
    assert torch.equal(host(R), torch.eye(3)[None])
    gen = torch.Generator().manual_seed(8401)
    from so3_log_ref import exp
    R0 = haar(1, gen)[0]
    cloud = (R0 @ exp(0.1 * torch.randn(500, 3, generator=gen, dtype=F64))).float()
    w = torch.rand(500, generator=gen)
    for weights in (None, w):
        got = host(lt.so3_mean(cloud.to(gpu_device), None if weights is None else weights.to(gpu_device)))
        want = ref.so3_mean(cloud, weights)
        assert (got.double() - want.double()).abs().max() <= 4 * 2.0 ** -24
    with pytest.raises(RuntimeError, match="no backward"):
        lt.so3_mean(cloud.to(gpu_device).requires_grad_(True))


# ------------------------------------------------------------------ alignment
@pytest.mark.parametrize("n", [300, 4099])
@pytest.mark.parametrize("angle", ref.PLANTED_ANGLES)
def test_alignment_noise_free(gpu_device, angle, n):
    """A G B against the fp64 solution on the same fp32 inputs: within 4x the fp32 restatement's
    own distance from it (max over samples of |A G_i B - (A G_i B)_64|_F)."""
    import lie_vae.lie_tools as lt
    Z, G, A0, B0 = ref.planted(n, angle, 0.0, 40 + int(angle), F32)
    A64, B64, _ = ref.align(Z.double(), G.double())
    P64 = A64 @ G.double() @ B64
    assert (P64 - Z.double()).flatten(1).norm(dim=-1).max() <= 1e-6  # the planted pair, up to fp32 rounding of Z
    A32, B32, _ = ref.align(Z, G)
    d_ref = ((A32 @ G @ B32).double() - P64).flatten(1).norm(dim=-1).max().item()
    A, B, rms = (host(t) for t in lt.align_rotations(Z.to(gpu_device), G.to(gpu_device)))
    assert A.dtype == F32 and A.shape == (3, 3) and B.shape == (3, 3) and rms.shape == ()
    d = ((A @ G @ B).double() - P64).flatten(1).norm(dim=-1).max().item()
    print(f"{angle:.0f} deg n={n}: |A G B - fp64| = {d:.2e} (restatement {d_ref:.2e}), rms {rms.item():.2e}")
    assert d <= 4 * d_ref
    assert ref.geodesic(A.double(), A0) <= 1e-5 and ref.geodesic(B.double(), B0) <= 1e-5
    assert rms.item() <= math.sqrt(16 * 2.0 ** -24 * 6)  # a difference of two numbers good to a few eps


@pytest.mark.parametrize("n", [300, 4099])
@pytest.mark.parametrize("angle", ref.PLANTED_ANGLES)
def test_alignment_noisy(gpu_device, angle, n):
    """0.05 rad of noise: the mean geodesic error is no larger than the planted pair's by more
    than 1 % (the least-squares pair fits the noise at least as well, up to chordal vs geodesic).
    rms = sqrt((6 wsum - 2 tr(B^T S)) / wsum): B's tangent error does not move the trace at the
    optimum, its distance from orthonormality (<= 8 eps) moves it by <= 2 * 8 eps * 3 wsum, i.e.
    48 * 2^-24 / 0.015 = 2e-4 of the residual (0.015 per sample at this noise) and half that of
    the rms: 2e-4 holds with a margin of two."""
    import lie_vae.lie_tools as lt
    Z, G, A0, B0 = ref.planted(n, angle, 0.05, 60 + int(angle), F32)
    A, B, rms = (host(t).double() for t in lt.align_rotations(Z.to(gpu_device), G.to(gpu_device)))
    got = ref.geodesic(Z.double(), A @ G.double() @ B).mean().item()
    planted = ref.geodesic(Z.double(), A0 @ G.double() @ B0).mean().item()
    res = ((Z.double() - A @ G.double() @ B) ** 2).sum((-1, -2)).mean().sqrt().item()
    print(f"{angle:.0f} deg n={n}: mean error {got:.5f} rad, planted pair {planted:.5f}, rms {rms.item():.5f}")
    assert got <= 1.01 * planted
    assert abs(rms.item() - res) <= 2e-4 * res


def test_one_sided_alignment_weights_and_graph_replay(gpu_device):
    """'left' / 'right' equal the closed-form (Kabsch) steps; a captured graph of the two-sided
    alignment replays to the eager result bit for bit."""
    import lie_vae.lie_tools as lt
    Z, G, A0, B0 = ref.planted(300, 150.0, 0.05, 77, F32)
    gen = torch.Generator().manual_seed(78)
    w = torch.rand(300, generator=gen) + 0.1
    Zg, Gg, wg = Z.to(gpu_device), G.to(gpu_device), w.to(gpu_device)
    Zd, Gd, wd = Z.double(), G.double(), w.double()
    A, B, rms = lt.align_rotations(Zg, Gg, side="left", weights=wg)
    want = ref.svd_project(torch.einsum("i,iab,icb->ac", wd, Zd, Gd))
    assert torch.equal(host(B), torch.eye(3)) and (host(A).double() - want).abs().max() <= 2.0 ** -23
    res = (wd * ((Zd - want @ Gd) ** 2).sum((-1, -2))).sum() / wd.sum()
    assert abs(rms.item() - res.sqrt().item()) <= 2e-4 * res.sqrt().item()
    A, B, rms = lt.align_rotations(Zg, Gg, side="right", weights=wg)
    want = ref.svd_project(torch.einsum("i,iba,ibc->ac", wd, Gd, Zd))
    assert torch.equal(host(A), torch.eye(3)) and (host(B).double() - want).abs().max() <= 2.0 ** -23
    # two-sided, weighted, against the fp64 restatement
    A, B, rms = (host(t) for t in lt.align_rotations(Zg, Gg, weights=wg))
    A64, B64, rms64 = ref.align(Zd, Gd, weights=wd)
    assert ((A @ G @ B).double() - A64 @ Gd @ B64).flatten(1).norm(dim=-1).max() <= 1e-5
    assert abs(rms.item() - rms64.item()) <= 2e-4 * rms64.item()
    # graph capture: no host sync, no host-to-device copy anywhere in the call
    eager = lt.align_rotations(Zg, Gg, weights=wg)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        lt.align_rotations(Zg, Gg, weights=wg)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lt.align_rotations(Zg, Gg, weights=wg)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ modules
def test_svd_mean_and_vae_step(gpu_device):
    import lie_vae.reparameterize as rp
    from lie_vae.experiments.vae import VAE
    torch.manual_seed(5)
    head = rp.SVDMean(10).to(gpu_device)
    x = torch.randn(33, 10, device=gpu_device)
    R = head(x)
    assert R.shape == (33, 3, 3)
    Rd = host(R).double()
    assert ((Rd.transpose(-1, -2) @ Rd - torch.eye(3, dtype=F64)).flatten(1).norm(dim=-1) <= 2e-6).all()
    assert ((torch.det(Rd) - 1).abs() <= 2e-6).all()
    model = VAE(latent_mode="so3", mean_mode="svd", decoder_mode="action", encode_mode="toy",
                deconv_mode="toy", degrees=3, rep_copies=4).to(gpu_device)
    xb = torch.randn(16, 16, 4, device=gpu_device)
    recon, kl, _ = model.elbo(xb, n=2)
    (recon.mean() + kl.mean()).backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert model.rep_group.mean_module.map.weight.grad.abs().max() > 0
    # mu_lie = the restatement on the same weights (the head's fp32 output, then the projection)
    h = model.encoder(xb)
    lin = model.rep_group.mean_module.map
    M = host(lin(h)).reshape(-1, 3, 3)
    mu = host(model.rep_group.mean_module(h))
    want, gamma = ref.svd_project(M), ref.svd_gamma(M)
    assert ((mu.double() - want).flatten(1).norm(dim=-1) * gamma <= FWD_BOUND_RAD).all()


def test_evaluate_poses_matches_the_restated_pipeline(gpu_device):
    """64 toy samples through an (untrained) svd-mean VAE: the four summary numbers against the
    same pipeline restated in fp64 on the host from the model's own posterior means, within the
    forward bound (4 x c_fwd x 2^-24 rad, in degrees)."""
    from lie_vae.experiments import pose_eval
    from lie_vae.experiments.datasets import ToyDataset
    from lie_vae.experiments.vae import VAE
    from oracle import lie_ref
    data = ToyDataset.generate(n=64, degrees=3, rep_copies=4, device=gpu_device, batch_size=32)
    q, _, x = data.tensors
    torch.manual_seed(6)
    model = VAE(latent_mode="so3", mean_mode="svd", decoder_mode="action", encode_mode="toy",
                deconv_mode="toy", degrees=3, rep_copies=4).to(gpu_device)
    got = pose_eval.evaluate_poses(model, x, q, batch_size=24)
    assert model.training
    Z = host(pose_eval.posterior_mean_rotations(model, x, batch_size=24)).double()
    G = lie_ref.quat_to_mat(host(q).double())
    A, B, _ = ref.align(Z, G)
    ang = torch.rad2deg(ref.geodesic(Z, A @ G @ B))
    s = torch.sort(ang).values
    want = {"mean_deg": ang.mean().item(), "median_deg": s[31].item(), "p90_deg": s[57].item(),
            "max_deg": s[63].item()}
    print(got, want)
    for k in want:
        assert abs(got[k] - want[k]) <= math.degrees(FWD_BOUND_RAD), k
    # matrices as ground truth, one-sided alignment, and a vmfq model's posterior mean
    got_m = pose_eval.evaluate_poses(model, x, G.float().to(gpu_device), batch_size=64, side="left")
    assert 0 <= got_m["mean_deg"] <= got_m["max_deg"] <= 180.0 + 1e-3
    vq = VAE(latent_mode="vmfq", decoder_mode="action", encode_mode="toy", deconv_mode="toy",
             degrees=3, rep_copies=4).to(gpu_device)
    got_q = pose_eval.evaluate_poses(vq, x, q)
    assert 0 <= got_q["median_deg"] <= got_q["p90_deg"] <= got_q["max_deg"] <= 180.0 + 1e-3
