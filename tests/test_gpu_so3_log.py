"""GPU checks of the SO(3) log map family (csrc/pointwise.hip so3_log_*, so3_rel_log_*,
so3_angle_*; lie_tools.so3_log / geodesic_distance / log_map; SO3reparameterize.log_prob)
against the fp64 restatement in tests/so3_log_ref.py, which tests/test_so3_log_cpu.py pins to
the reference's fp64 log_map, scipy and central differences.  Each band holds 257 rotations
(one 256-thread block and a tail); the bands are the exact identity, theta in [1e-7, 1e-3],
[1e-3, 0.1], [0.1, 3], [3, pi - 1e-3], [pi - 1e-3, pi) and exact half-turns."""
import math

import numpy as np
import pytest
import torch

import so3_log_ref as ref
from conftest import golden

pytestmark = pytest.mark.gpu
F64 = torch.float64
SIGNED = ("near_pi", "half_turn")        # v is compared up to sign (both are logs at pi)
SMOOTH = ref.BANDS[:5]                   # bands whose gradients are compared, not only finite


def host(t):
    return t.detach().cpu()


def up_to_sign(v, v64, name):
    d = (v.double() - v64).norm(dim=-1)
    return torch.minimum(d, (v.double() + v64).norm(dim=-1)) if name in SIGNED else d


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", ref.BANDS)
def test_log_forward_fp32(gpu_device, name):
    """Round trip |exp64(v) - R|_F <= 1e-5 |R|_F per sample; against the fp64 restatement on
    the same fp32 R, |v - v64| <= 1e-5 |v64| + 1e-6 (1e-6: ~10 ulp of the matrix entries, how
    far a rounded fp32 R lies from SO(3)); no NaN; the identity gives exactly 0."""
    import lie_vae.lie_tools as lt
    case = ref.band_case(name)
    v = host(lt.so3_log(case["R"].to(gpu_device)))
    assert v.dtype == torch.float32 and v.shape == (ref.BAND_N, 3)
    assert torch.isfinite(v).all()
    err, scale = ref.normwise(ref.exp(v.double()), case["R"].double())
    dv = up_to_sign(v, case["v64"], name)
    bound = 1e-5 * case["v64"].norm(dim=-1) + 1e-6
    print(f"{name}: round trip {float((err / scale).max()):.2e}, |v - v64| max {float(dv.max()):.2e}, "
          f"worst dv / bound {float((dv / bound).max()):.3f}")
    assert (err <= 1e-5 * scale).all()
    assert (dv <= bound).all()
    assert (v.norm(dim=-1) <= math.pi * (1 + 1e-6)).all()
    if name == "identity":
        assert torch.equal(v, torch.zeros_like(v))
    if name == "half_turn":
        assert (v.abs().max(-1).values - v.max(-1).values <= 1e-6).all()  # largest component > 0


def test_log_forward_golden(gpu_device):
    """The reference's own matrices (fp64 rodrigues, rounded to fp32) against its fp64 log_map."""
    import lie_vae.lie_tools as lt
    g = golden("so3_log.npz")
    R, v64 = torch.from_numpy(g["R"]), torch.from_numpy(g["v64"])
    v = host(lt.so3_log(R.float().to(gpu_device)))
    dv = (v.double() - v64).norm(dim=-1)
    theirs = (torch.from_numpy(g["v32_ref"]).double() - v64).norm(dim=-1)
    print(f"golden: |v - v64| max {float(dv.max()):.2e} (reference fp32 expression {float(theirs.max()):.2e})")
    assert (dv <= 1e-5 * v64.norm(dim=-1) + 1e-6).all()
    # batched log_map: the same values as skew matrices
    X = lt.log_map(R.float().to(gpu_device))
    assert X.shape == (256, 3, 3)
    assert torch.equal(host(X), lt.map_to_lie_algebra(v))


@pytest.mark.parametrize("name", ref.BANDS)
def test_log_fp64_twin(gpu_device, name):
    """fp64 in, fp64 kernels: 1e-12 max(|v|, 1) on v; gR at 1e-10 max(|g|, 1) in the smooth
    bands, finite in the two pi bands."""
    import lie_vae.lie_tools as lt
    R = ref.band(name)[0]
    v64, th64, _ = ref.log_polar(R)
    gen = torch.Generator().manual_seed(21)
    gv = torch.randn(R.shape[0], 3, generator=gen, dtype=F64)
    Rg = R.to(gpu_device).requires_grad_(True)
    v = lt.so3_log(Rg)
    assert v.dtype == F64
    (v * gv.to(gpu_device)).sum().backward()
    dv = up_to_sign(host(v), v64, name)
    print(f"{name}: fp64 |v - v64| max {float(dv.max()):.2e}")
    assert (dv <= 1e-12 * v64.norm(dim=-1).clamp(min=1.0)).all()
    g = host(Rg.grad)
    assert g.dtype == F64 and torch.isfinite(g).all()
    if name in SMOOTH:
        want = ref.log_vjp(R, gv)
        err = (g - want).abs().max().item()
        print(f"{name}: fp64 |gR - gR64| max {err:.2e}")
        assert err <= 1e-10 * max(float(want.abs().max()), 1.0)


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", ref.BANDS)
def test_log_backward_fp32(gpu_device, name):
    """gR against the restatement's R hat(J_r^-T gv / 2), normwise 1e-5 in the first five bands;
    R^T gR skew to 1e-6 |gR|; finite in every band."""
    import lie_vae.lie_tools as lt
    case = ref.band_case(name)
    Rg = case["R"].to(gpu_device).requires_grad_(True)
    (lt.so3_log(Rg) * case["gv"].to(gpu_device)).sum().backward()
    g = host(Rg.grad)
    assert g.dtype == torch.float32 and torch.isfinite(g).all()
    M = case["R"].double().transpose(-1, -2) @ g.double()
    sym = (0.5 * (M + M.transpose(-1, -2))).flatten(1).norm(dim=-1)
    gn = g.double().flatten(1).norm(dim=-1)
    print(f"{name}: |sym(R^T gR)| / |gR| max {float((sym / gn).max()):.2e}")
    assert (sym <= 1e-6 * gn).all()
    if name in SMOOTH:
        err, scale = ref.normwise(g, case["gR64"])
        print(f"{name}: gR normwise max {float((err / scale).max()):.2e}")
        assert (err <= 1e-5 * scale).all()


def test_log_autograd_end_to_end_fp64(gpu_device):
    """A quaternion leaf through quaternions_to_group_matrix and so3_log on the device, against
    CPU autograd of the reference's acos / sin expression, at the golden's angles; 1e-10."""
    import lie_vae.lie_tools as lt
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(22)
    v0 = torch.from_numpy(golden("so3_log.npz")["v64"])
    th = v0.norm(dim=-1, keepdim=True)
    q0 = torch.cat([torch.sin(th / 2) * v0 / th, torch.cos(th / 2)], -1)
    q0 = q0 * (0.5 + torch.rand(len(q0), 1, generator=gen, dtype=F64))
    gv = torch.randn(len(q0), 3, generator=gen, dtype=F64)
    qc = q0.clone().requires_grad_(True)
    vc = torch.stack([lie_ref.vee(lie_ref.so3_log(r)) for r in lie_ref.quat_to_mat(qc)])
    (vc * gv).sum().backward()
    qg = q0.to(gpu_device).requires_grad_(True)
    vg = lt.so3_log(lt.quaternions_to_group_matrix(qg))
    (vg * gv.to(gpu_device)).sum().backward()
    assert (host(vg) - vc.detach()).abs().max() <= 1e-12 * math.pi
    err = (host(qg.grad) - qc.grad).abs().max().item()
    print(f"end-to-end fp64 gradient: max {err:.2e} of {float(qc.grad.abs().max()):.2e}")
    assert err <= 1e-10 * max(float(qc.grad.abs().max()), 1.0)


# ------------------------------------------------------------------ relative log
def _rel_case(ns, B):
    gen = torch.Generator().manual_seed(500 + 7 * ns + B)
    mu = ref.haar(B, gen, torch.float32)
    u = torch.randn(ns, B, 3, generator=gen, dtype=F64)
    th = 0.1 + 2.9 * torch.rand(ns, B, 1, generator=gen, dtype=F64)
    v = (u / u.norm(dim=-1, keepdim=True) * th).float()
    return mu, v, torch.randn(ns, B, 3, generator=gen)


@pytest.mark.parametrize("ns,B", [(1, 1), (3, 5), (2, 257)])
def test_rel_log_inverts_so3_sample(gpu_device, ns, B):
    """z = so3_sample(mu, v) on the device, |v| in [0.1, 3]; rel_log(mu, z) against the fp64
    restatement on the same fp32 (mu, z) under the forward bound, and against v itself.  The
    latter bound: z carries the sampler's error, within the project's normwise 1e-5 |z|_F =
    1.7e-5, which the log (|J_r^-1| <= pi/2 on a tangent vector of norm |dz|_F / sqrt 2)
    passes on as at most 1.9e-5, on top of the forward bound.  gmu and gz against the
    restatement, normwise 1e-5; gmu bitwise equal across two runs."""
    import lie_vae._ops as ops
    mu, v, gv = _rel_case(ns, B)
    mug = mu.to(gpu_device).requires_grad_(True)
    with torch.no_grad():
        z = ops.so3_sample(mug, v.to(gpu_device))
    zg = z.clone().requires_grad_(True)
    out = ops.so3_rel_log(mug, zg)
    assert out.shape == (ns, B, 3) and out.dtype == torch.float32
    (out * gv.to(gpu_device)).sum().backward()
    z64, mu64 = host(z).double(), mu.double()
    want = ref.rel_log(mu64, z64)
    dv = (host(out).double() - want).norm(dim=-1)
    back = (host(out).double() - v.double()).norm(dim=-1)
    fwd_bound = 1e-5 * want.norm(dim=-1) + 1e-6
    print(f"({ns},{B}): |v' - v64| max {float(dv.max()):.2e}, |v' - v| max {float(back.max()):.2e}")
    assert (dv <= fwd_bound).all()
    assert (back <= fwd_bound + 1.9e-5).all()
    gmu64, gz64 = ref.rel_log_vjp(mu64, z64, gv.double())
    for got, ref64, what in ((mug.grad, gmu64, "gmu"), (zg.grad, gz64, "gz")):
        err = (host(got).double() - ref64).flatten(-2).norm(dim=-1)
        scale = ref64.flatten(-2).norm(dim=-1)
        print(f"({ns},{B}): {what} normwise max {float((err / scale).max()):.2e}")
        assert (err <= 1e-5 * scale).all(), what
    first = mug.grad.clone()
    mug.grad = None
    (ops.so3_rel_log(mug, zg) * gv.to(gpu_device)).sum().backward()
    assert torch.equal(first, mug.grad)


def test_rel_log_fp64_and_empty(gpu_device):
    import lie_vae._ops as ops
    mu, v, gv = _rel_case(3, 5)
    mu64 = ref.haar(5, torch.Generator().manual_seed(23))
    z64 = mu64 @ ref.exp(v.double())
    mug = mu64.to(gpu_device).requires_grad_(True)
    zg = z64.to(gpu_device).requires_grad_(True)
    out = ops.so3_rel_log(mug, zg)
    assert out.dtype == F64
    (out * gv.double().to(gpu_device)).sum().backward()
    assert (host(out) - v.double()).abs().max() <= 1e-12 * math.pi
    gmu64, gz64 = ref.rel_log_vjp(mu64, z64, gv.double())
    assert (host(mug.grad) - gmu64).abs().max() <= 1e-10 * max(float(gmu64.abs().max()), 1.0)
    assert (host(zg.grad) - gz64).abs().max() <= 1e-10 * max(float(gz64.abs().max()), 1.0)
    # no samples: an empty v, and gmu zero-filled
    m32 = mu.to(gpu_device).requires_grad_(True)
    empty = ops.so3_rel_log(m32, torch.empty(0, 5, 3, 3, device=gpu_device))
    assert empty.shape == (0, 5, 3)
    empty.sum().backward()
    assert torch.equal(host(m32.grad), torch.zeros(5, 3, 3))


# ------------------------------------------------------------------ angle
def _angle_pairs(name):
    gen = torch.Generator().manual_seed(600 + ref.BANDS.index(name))
    A = ref.haar(ref.BAND_N, gen)
    return A.float(), (A @ ref.band(name)[0]).float()


@pytest.mark.parametrize("name", ref.BANDS)
def test_angle_forward(gpu_device, name):
    """|theta - theta64| <= 1e-5 theta64 + 1e-6 against the restatement on the same fp32 pair;
    symmetric in (A, B) bit for bit; in [0, pi]."""
    import lie_vae.lie_tools as lt
    A, B = _angle_pairs(name)
    Ag, Bg = A.to(gpu_device), B.to(gpu_device)
    th = host(lt.geodesic_distance(Ag, Bg))
    th64 = ref.angle(A.double(), B.double())
    d = (th.double() - th64).abs()
    print(f"{name}: |theta - theta64| max {float(d.max()):.2e}")
    assert th.shape == (ref.BAND_N,) and torch.isfinite(th).all()
    assert (d <= 1e-5 * th64 + 1e-6).all()
    assert ((th >= 0) & (th <= math.pi * (1 + 1e-7))).all()
    assert torch.equal(th, host(lt.geodesic_distance(Bg, Ag)))
    if name == "identity":
        assert torch.equal(th, torch.zeros_like(th))


def test_angle_of_a_rotation_with_itself_is_zero_with_zero_gradient(gpu_device):
    import lie_vae.lie_tools as lt
    A = ref.haar(ref.BAND_N, torch.Generator().manual_seed(24), torch.float32)
    Ag = A.to(gpu_device).requires_grad_(True)
    Bg = A.to(gpu_device).requires_grad_(True)
    th = lt.geodesic_distance(Ag, Bg)
    th.sum().backward()
    assert torch.equal(host(th), torch.zeros(ref.BAND_N))
    assert torch.equal(host(Ag.grad), torch.zeros_like(A)) and torch.equal(host(Bg.grad), torch.zeros_like(A))


@pytest.mark.parametrize("name", ["mid", "large"])
def test_angle_backward(gpu_device, name):
    """gA and gB against the restatement, normwise 1e-5, fp32 and fp64.  Bands with
    sin(theta) >= 1e-3: the fp32 product A^T B carries ~1e-7 per entry, and the axis the
    gradient points along is that error over sin(theta) away where cos >= 0 (the gradient of a
    norm near its kink), so below theta = 0.1 an fp32 evaluation cannot meet 1e-5; `mid` starts
    there, and at theta = 0.1 the axis is good to ~2e-6."""
    import lie_vae.lie_tools as lt
    A, B = _angle_pairs(name)
    gth = torch.randn(ref.BAND_N, generator=torch.Generator().manual_seed(25))
    for dt, tol in ((torch.float32, 1e-5), (F64, 1e-10)):
        if dt == F64:
            A, B = A.double(), B.double()
            A, B = ref.exp(ref.log_polar(A)[0]), ref.exp(ref.log_polar(B)[0])  # back onto SO(3)
        Ag, Bg = A.to(gpu_device).requires_grad_(True), B.to(gpu_device).requires_grad_(True)
        (lt.geodesic_distance(Ag, Bg) * gth.to(dt).to(gpu_device)).sum().backward()
        gA64, gB64 = ref.angle_vjp(A.double(), B.double(), gth.double())
        for got, want, what in ((Ag.grad, gA64, "gA"), (Bg.grad, gB64, "gB")):
            assert got.dtype == dt
            err, scale = ref.normwise(host(got), want)
            print(f"{name} {dt}: {what} normwise max {float((err / scale).max()):.2e}")
            assert (err <= tol * scale).all(), (what, dt)


# ------------------------------------------------------------------ log_prob
def _log_prob_setup(gpu_device, lo, hi, n=2, B=33):
    """An SO3reparameterize with a quaternion mean head, sigma = softplus(linear) in [0.2, 1]
    and eps chosen so that |v| = |eps sigma| is uniform in [lo, hi]."""
    import lie_vae.reparameterize as rp
    torch.manual_seed(31)
    rep = rp.SO3reparameterize(rp.N0reparameterize(10, z_dim=3), rp.QuaternionMean(10), k=10)
    gen = torch.Generator().manual_seed(32)
    with torch.no_grad():
        rep.reparameterize.sigma_linear.weight.copy_(0.08 * torch.randn(3, 10, generator=gen))
        rep.reparameterize.sigma_linear.bias.fill_(-0.5)
    h = torch.randn(B, 10, generator=gen)
    sigma = torch.nn.functional.softplus(rep.reparameterize.sigma_linear(h)).detach()
    assert sigma.min() >= 0.2 and sigma.max() <= 1.0, (sigma.min(), sigma.max())
    u = torch.randn(n, B, 3, generator=gen)
    th = lo + (hi - lo) * torch.rand(n, B, 1, generator=gen)
    eps = u / u.norm(dim=-1, keepdim=True) * th / sigma
    return rep, h, eps


def _restated_grads(rep, h, qz, gout, dtype):
    """Gradients of sum(gout * log_prob) to h, sigma and qz from the restatement in `dtype` on
    the CPU: the mean head and softplus as torch ops, then so3_log_ref.log_prob."""
    from oracle import lie_ref
    p = {k: t.detach().to(dtype) for k, t in rep.state_dict().items()}
    hh = h.detach().to(dtype).requires_grad_(True)
    qq = qz.detach().to(dtype).requires_grad_(True)
    mu = lie_ref.quat_to_mat(hh @ p["mean_module.map.weight"].T + p["mean_module.map.bias"])
    sigma = torch.nn.functional.softplus(
        hh @ p["reparameterize.sigma_linear.weight"].T + p["reparameterize.sigma_linear.bias"])
    lp = ref.log_prob(mu, lie_ref.quat_to_mat(qq), sigma, 10)
    # h feeds both heads: its gradient holds the mean's and sigma's paths, on the device as here
    return lp.detach(), torch.autograd.grad((lp * gout.to(dtype)).sum(), (hh, sigma, qq))


LOG_PROB_RANGES = {"inside": (0.05, math.pi - 0.1), "wrapped": (math.pi + 1e-3, 2 * math.pi - 0.5)}


@pytest.mark.parametrize("which", list(LOG_PROB_RANGES))
def test_log_prob(gpu_device, which):
    """rep.log_prob(rep.z) against rep.log_posterior() at rtol 1e-5, atol 1e-4 (the existing
    log-posterior tolerance), with |v| < pi - 0.1 and with |v| in (pi, 2 pi - 0.5), where the
    log returns the short way round and the sheets make up for it.  Gradients of
    sum(g * log_prob(z)) to the mean head's input, to sigma and to a quaternion parametrising
    z, against fp64 autograd of the restatement: bounded by 4x the error of the restatement
    itself evaluated in fp32 on the CPU against its fp64 value on the same inputs (whole-tensor
    norms; 4: a different but valid operation order), never against the code under test.
    Measured on an MI355X, kernel error / restatement-fp32 error, relative to |g64|:
      inside:  dh 7.9e-7 / 1.1e-6, dsigma 4.2e-7 / 2.1e-7, dq 1.1e-6 / 1.6e-6
      wrapped: dh 5.0e-7 / 2.9e-7, dsigma 5.5e-7 / 1.5e-7, dq 6.2e-7 / 2.8e-7
    (the closest to its bound is dsigma of `wrapped`, at 3.7 of the allowed 4)."""
    from oracle import lie_ref
    lo, hi = LOG_PROB_RANGES[which]
    rep, h, eps = _log_prob_setup(gpu_device, lo, hi)
    rep = rep.to(gpu_device)
    hg = h.to(gpu_device).requires_grad_(True)
    z = rep(hg, eps.shape[0], eps=eps.to(gpu_device))
    vn = host(rep.v).norm(dim=-1)
    assert (vn > lo - 1e-4).all() and (vn < hi + 1e-4).all()
    lp_z, lp_post = host(rep.log_prob(z)), host(rep.log_posterior())
    assert lp_z.shape == tuple(eps.shape[:2])
    print(f"{which}: |log_prob(z) - log_posterior| max {float((lp_z - lp_post).abs().max()):.2e}")
    np.testing.assert_allclose(lp_z.numpy(), lp_post.numpy(), rtol=1e-5, atol=1e-4)
    assert torch.equal(host(rep.log_prob(z[0])), lp_z[:1])  # (B,3,3) -> (1,B)
    # gradients at z given by a quaternion leaf
    gen = torch.Generator().manual_seed(33)
    qz = lie_ref.mat_to_quat(host(z).double()) * (0.5 + torch.rand(*eps.shape[:2], 1, generator=gen, dtype=F64))
    qz = qz.float()
    gout = torch.randn(*eps.shape[:2], generator=gen)
    import lie_vae.lie_tools as lt
    qg = qz.to(gpu_device).requires_grad_(True)
    lp = rep.log_prob(lt.quaternions_to_group_matrix(qg))
    sigma = rep.reparameterize.sigma
    gh, gs, gq = torch.autograd.grad((lp * gout.to(gpu_device)).sum(), (hg, sigma, qg))
    lp64, g64 = _restated_grads(rep.cpu(), h, qz, gout, F64)
    lp32, g32 = _restated_grads(rep, h, qz, gout, torch.float32)
    np.testing.assert_allclose(host(lp).numpy(), lp64.numpy(), rtol=1e-5, atol=1e-4)
    for got, w64, w32, what in zip((gh, gs, gq), g64, g32, ("dh", "dsigma", "dq")):
        err = (host(got).double() - w64).norm().item()
        own = (w32.double() - w64).norm().item()
        print(f"{which}: {what} |g - g64| / |g64| = {err / w64.norm().item():.2e}, the restatement in "
              f"fp32: {own / w64.norm().item():.2e}")
        assert torch.isfinite(got).all()
        assert err <= 4 * own, (what, err, own)


# ------------------------------------------------------------------ shapes, graph
def test_leading_shapes_and_strides(gpu_device):
    import lie_vae.lie_tools as lt
    R = ref.band("mid")[0][:30].float().to(gpu_device)
    flat = lt.so3_log(R)
    assert lt.so3_log(R[0]).shape == (3,) and torch.equal(lt.so3_log(R[0]), flat[0])
    assert torch.equal(lt.so3_log(R[:5]), flat[:5])
    assert torch.equal(lt.so3_log(R[:6].reshape(2, 3, 3, 3)), flat[:6].reshape(2, 3, 3))
    assert torch.equal(lt.log_map(R[:6].reshape(2, 3, 3, 3)),
                       lt.map_to_lie_algebra(flat[:6]).reshape(2, 3, 3, 3))
    # non-contiguous: every other matrix, and a transposed view (the inverse rotation: -v up to rounding)
    assert torch.equal(lt.so3_log(R[::2]), flat[::2])
    Rt = R.transpose(-1, -2)
    assert not Rt.is_contiguous()
    assert torch.equal(lt.so3_log(Rt), lt.so3_log(Rt.contiguous()))
    assert (lt.so3_log(Rt) + flat).abs().max() <= 1e-6
    A, B = R[:6], R[6:12]
    d = lt.geodesic_distance(A, B)
    assert lt.geodesic_distance(A[0], B[0]).shape == () and torch.equal(lt.geodesic_distance(A[0], B[0]), d[0])
    assert torch.equal(lt.geodesic_distance(A.reshape(2, 3, 3, 3), B.reshape(2, 3, 3, 3)), d.reshape(2, 3))
    assert torch.equal(lt.geodesic_distance(R[0:12:2], R[1:12:2]),
                       lt.geodesic_distance(R[0:12:2].contiguous(), R[1:12:2].contiguous()))
    # a stride-0 expand (one rotation against a batch)
    assert torch.equal(lt.geodesic_distance(A[:1].expand(6, 3, 3), B),
                       lt.geodesic_distance(A[:1].repeat(6, 1, 1), B))


def test_log_graph_capture_matches_eager(gpu_device):
    """so3_log forward and backward captured once and replayed: bitwise the eager results."""
    import lie_vae.lie_tools as lt
    R = torch.cat([ref.band_case(n)["R"][:40] for n in ref.BANDS]).to(gpu_device).requires_grad_(True)
    gv = torch.randn(R.shape[0], 3, device=gpu_device)
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        v = lt.so3_log(R)
        v.backward(gv)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    eager = (v.detach().clone(), R.grad.clone())
    R.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        v_g = lt.so3_log(R)
        v_g.backward(gv)
    g.replay()
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(v_g, eager[0]) and torch.equal(R.grad, eager[1])
