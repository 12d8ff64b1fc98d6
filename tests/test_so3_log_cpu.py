"""CPU checks of the SO(3) log map family (csrc/so3_device.h so3_log_polar, lie_tools.so3_log /
geodesic_distance / log_map, SO3reparameterize.log_prob): the twelve C entry points and their
argument checks (no device needed: the checks run before any launch), the refusal of CPU
tensors, and the fp64 restatement in tests/so3_log_ref.py against independent facts: the
reference's own fp64 log_map (tests/golden/so3_log.npz), scipy's rotation vectors, the
round trip through the exponential, central differences, the identity and exact half-turns.
The restatement in fp32 gives the error the algorithm itself has in that format."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import so3_log_ref as ref
from conftest import REPO, golden

F64 = torch.float64
BASE = ("lv_so3_log_fwd", "lv_so3_log_bwd", "lv_so3_rel_log_fwd", "lv_so3_rel_log_bwd",
        "lv_so3_angle_fwd", "lv_so3_angle_bwd")
ENTRY_POINTS = BASE + tuple(n + "_f64" for n in BASE)


def test_library_exports_the_log_entry_points():
    from lie_vae import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "lievae.h")).read()
    declared = set(re.findall(r"\b(lv_\w+)\s*\(", header))
    assert len(ENTRY_POINTS) == 12
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
        assert name in declared, name
    assert "lie_tools.py:100-109" in header
    assert lib.lv_abi_version() == 1


def test_argument_checks_before_any_launch():
    """Negative sizes and null pointers with work to do return LV_ERR_ARG with a message before
    anything is launched (dummy non-null pointers, no device); empty sizes are LV_OK."""
    from lie_vae import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(16)  # never dereferenced: the checks run first

    def refused(rc, word):
        msg = lib.lv_last_error()
        assert rc == -1 and msg and word in msg, (rc, msg)

    for suf in ("", "_f64"):
        lf, lb = getattr(lib, "lv_so3_log_fwd" + suf), getattr(lib, "lv_so3_log_bwd" + suf)
        rf, rb = getattr(lib, "lv_so3_rel_log_fwd" + suf), getattr(lib, "lv_so3_rel_log_bwd" + suf)
        af, ab = getattr(lib, "lv_so3_angle_fwd" + suf), getattr(lib, "lv_so3_angle_bwd" + suf)
        refused(lf(P, P, -1, None), b"n must")
        refused(lb(P, P, P, -1, None), b"n must")
        refused(af(P, P, P, -3, None), b"n must")
        refused(ab(P, P, P, P, P, -1, None), b"n must")
        refused(lf(None, None, -1, None), b"n must")  # the size first, also with null pointers
        for ns, B in ((-1, 4), (4, -1), (-2, -2)):
            refused(rf(P, P, P, ns, B, None), b"ns and B")
            refused(rb(P, P, P, P, P, ns, B, None), b"ns and B")
        for fn, k, tail in ((lf, 2, (5,)), (lb, 3, (5,)), (af, 3, (5,)), (ab, 5, (5,)),
                            (rf, 3, (2, 3)), (rb, 5, (2, 3))):
            for i in range(k):
                a = [P] * k
                a[i] = None
                refused(fn(*a, *tail, None), b"null")
        # ns == 0 with B > 0 still writes gmu: mu and gmu are needed, the per-sample ones not
        refused(rb(P, None, None, None, None, 0, 3, None), b"null")
        # empty sizes: LV_OK, nothing launched (null pointers are then fine too)
        assert lf(P, P, 0, None) == 0 and lf(None, None, 0, None) == 0
        assert lb(P, P, P, 0, None) == 0 and lb(None, None, None, 0, None) == 0
        assert af(P, P, P, 0, None) == 0 and ab(None, None, None, None, None, 0, None) == 0
        for ns, B in ((0, 5), (5, 0), (0, 0)):
            assert rf(P, P, P, ns, B, None) == 0
            assert rf(None, None, None, ns, B, None) == 0
        for ns, B in ((5, 0), (0, 0)):
            assert rb(P, P, P, P, P, ns, B, None) == 0
            assert rb(None, None, None, None, None, ns, B, None) == 0


def test_cpu_tensors_fail_loudly_and_unbatched_log_map_is_unchanged():
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    import lie_vae.reparameterize as rp
    from oracle import lie_ref
    assert "so3_log" in lt.__all__ and "geodesic_distance" in lt.__all__
    gen = torch.Generator().manual_seed(3)
    R = ref.haar(6, gen, torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.so3_log(R)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.so3_log(R[0].double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.geodesic_distance(R[:3], R[3:])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.log_map(R)  # batched: the kernel's path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.so3_rel_log(R[:3], R.reshape(2, 3, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.so3_angle(R, R)
    rep = rp.SO3reparameterize(rp.N0reparameterize(10, z_dim=3), rp.QuaternionMean(10), k=10)
    rep.mu_lie, rep.reparameterize.sigma = R[:3], torch.rand(3, 3) + 0.2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rep.log_prob(R.reshape(2, 3, 3, 3))
    with pytest.raises(AssertionError):
        lt.so3_log(torch.randn(4, 3, 2))
    with pytest.raises(AssertionError, match="mu must"):
        ops.so3_rel_log(R[:2], R.reshape(2, 3, 3, 3))
    with pytest.raises(AssertionError, match="one shape"):
        ops.so3_angle(R[:2], R)
    # a single matrix: the reference's tensor expression, on the CPU, bit for bit
    for dt in (torch.float32, F64):
        for k in range(6):
            assert torch.equal(lt.log_map(R[k].to(dt)), lie_ref.so3_log(R[k].to(dt)))


# ------------------------------------------------------------ restatement vs facts
def test_restatement_against_reference_fp64_log_map():
    """tests/golden/so3_log.npz: the reference's rodrigues and log_map in fp64 at 256 angles in
    [0.05, pi - 0.05]; 1e-12."""
    g = golden("so3_log.npz")
    R, v64 = torch.from_numpy(g["R"]), torch.from_numpy(g["v64"])
    assert R.shape == (256, 3, 3) and R.dtype == F64 and g["v32_ref"].dtype == np.float32
    v, th, a = ref.log_polar(R)
    err = (v - v64).abs().max().item()
    print(f"restatement vs reference fp64 log_map: max |dv| = {err:.2e}")
    assert err <= 1e-12
    assert (th - v64.norm(dim=-1)).abs().max() <= 1e-12
    assert ((a.norm(dim=-1) - 1).abs() <= 1e-14).all()


def test_restatement_against_scipy_rotvec():
    for name in ("small", "mid", "large"):
        R = ref.band(name)[0]
        want = torch.from_numpy(Rotation.from_matrix(R.numpy()).as_rotvec())
        err = (ref.log_polar(R)[0] - want).norm(dim=-1).max().item()
        print(f"{name}: restatement vs scipy as_rotvec, max |dv| = {err:.2e}")
        assert err <= 1e-12 * math.pi


@pytest.mark.parametrize("name", ref.BANDS)
def test_restatement_round_trip_and_angles(name):
    """exp(log R) = R to 1e-12 normwise in fp64 in every band, theta and the axis as drawn
    (up to sign at pi), theta in [0, pi]."""
    R, a, th = ref.band(name)
    assert R.shape == (ref.BAND_N, 3, 3)
    v, t, ax = ref.log_polar(R)
    assert torch.isfinite(v).all()
    err, scale = ref.normwise(ref.exp(v), R)
    print(f"{name}: exp(log R) - R normwise max {float((err / scale).max()):.2e}")
    assert (err <= 1e-12 * scale).all()
    assert ((t >= 0) & (t <= math.pi)).all()
    assert ((t - th).abs() <= 1e-12).all()  # atan2 of (sin, cos) is well conditioned throughout
    if name == "identity":
        assert torch.equal(v, torch.zeros_like(v)) and torch.equal(ax, torch.zeros_like(ax))
    elif name == "half_turn":
        assert ((v.norm(dim=-1) - math.pi).abs() <= 1e-14).all()
        # the sign rule: the component of largest magnitude is positive (ties up to rounding:
        # the largest positive component is as large as the largest magnitude)
        assert (v.abs().max(-1).values - v.max(-1).values <= 1e-14).all()
        assert (torch.minimum((ax - a).norm(dim=-1), (ax + a).norm(dim=-1)) <= 1e-14).all()
    else:
        tol = 1e-9 if name in ("tiny", "near_pi") else 1e-12  # axis from a 1e-7 / 1e-9 sine
        assert ((ax - a).norm(dim=-1) <= tol).all()


def test_half_turn_ties_are_deterministic():
    """Coordinate axes and ties between components: still a unit axis and a valid log."""
    ax = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1, 1, 0], [1, -1, 0], [-1, -1, -1],
                       [0, 1, -1]], dtype=F64)
    ax = ax / ax.norm(dim=-1, keepdim=True)
    R = 2 * ax[:, :, None] * ax[:, None, :] - torch.eye(3, dtype=F64)
    v, th, a = ref.log_polar(R)
    assert torch.equal(th, torch.full_like(th, math.pi))
    assert ((ref.exp(v) - R).flatten(1).norm(dim=-1) <= 1e-14).all()
    assert torch.equal(a[0], torch.tensor([1.0, 0, 0], dtype=F64))
    # the first of equal components is the positive one
    assert a[3, 0] > 0 and a[4, 0] > 0 and a[4, 1] < 0 and (a[5] > 0).all() and a[6, 1] > 0


@pytest.mark.parametrize("name", ["tiny", "small", "mid", "large"])
def test_jr_inv_against_central_differences(name):
    """J_r^-1 column j against (log(R exp(h e_j)) - log(R exp(-h e_j))) / 2h, h = 1e-6, in fp64.
    The difference quotient rounds at eps |v| / h <= 2.2e-16 * pi / 1e-6 = 7e-10 per entry and
    truncates at h^2 = 1e-12 times a third derivative; the bound is 1e-8."""
    R = ref.band(name)[0][:64]
    v = ref.log_polar(R)[0]
    J = ref.jr_inv(v)
    h = 1e-6
    cols = []
    for j in range(3):
        e = torch.zeros(R.shape[0], 3, dtype=F64)
        e[:, j] = h
        cols.append((ref.log_polar(R @ ref.exp(e))[0] - ref.log_polar(R @ ref.exp(-e))[0]) / (2 * h))
    err = (J - torch.stack(cols, -1)).abs().max().item()
    print(f"{name}: J_r^-1 vs central differences, max {err:.2e}")
    assert err <= 1e-8
    # the tangent gradient pairs with it: <gR, R hat(xi)> = <gv, J_r^-1 xi>
    gen = torch.Generator().manual_seed(9)
    gv, xi = torch.randn(2, R.shape[0], 3, generator=gen, dtype=F64)
    lhs = (ref.log_vjp(R, gv) * (R @ ref.hat(xi))).sum((-1, -2))
    rhs = (gv * (J @ xi[..., None])[..., 0]).sum(-1)
    assert ((lhs - rhs).abs() <= 1e-13 * (1 + rhs.abs())).all()


def test_kappa_limits_and_series_seam():
    # either side of the seam, 2e-12 apart (kappa' = theta / 360 there: 1e-15 of slope)
    th = torch.tensor([0.0, 1e-8, ref.SERIES_TH - 1e-12, ref.SERIES_TH + 1e-12, math.pi], dtype=F64)
    k = ref.kappa(th)
    assert k[0] == 1 / 12 and abs(k[1] - 1 / 12) < 1e-16
    assert abs(k[2] - k[3]) <= 1e-14 and abs(k[4] - 1 / math.pi ** 2) <= 1e-16
    s = torch.tensor([ref.SERIES_S - 1e-9, ref.SERIES_S + 1e-9], dtype=F64)
    series = 1 + s ** 2 * (1 / 6 + s ** 2 * (3 / 40 + s ** 2 * (15 / 336)))
    # the first term left out is 35/1152 s^8 = 2.0e-14 at the seam, far inside the fp64 bar 1e-12
    assert ((series - torch.asin(s) / s).abs() <= 35 / 1152 * 0.03 ** 8 * 1.5).all()


def test_log_autograd_matches_reference_expression():
    """The tangent gradient composed with a parametrisation that stays in SO(3) (a quaternion)
    equals fp64 autograd through the reference's acos / sin expression."""
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(12)
    g = golden("so3_log.npz")
    v0 = torch.from_numpy(g["v64"])[:32]
    th = v0.norm(dim=-1, keepdim=True)
    q0 = torch.cat([torch.sin(th / 2) * v0 / th, torch.cos(th / 2)], -1) * 1.7
    gv = torch.randn(32, 3, generator=gen, dtype=F64)
    qa = q0.clone().requires_grad_(True)
    (ref.log(lie_ref.quat_to_mat(qa)) * gv).sum().backward()
    qb = q0.clone().requires_grad_(True)
    vb = torch.stack([lie_ref.vee(lie_ref.so3_log(r)) for r in lie_ref.quat_to_mat(qb)])
    (vb * gv).sum().backward()
    err = (qa.grad - qb.grad).abs().max().item()
    print(f"tangent gradient vs autograd of the reference expression: max {err:.2e}")
    assert err <= 1e-10 * max(qb.grad.abs().max().item(), 1.0)


def test_rel_log_and_angle_restatement_vjps_against_autograd():
    """rel_log_vjp / angle_vjp (the kernels' contracts) against fp64 autograd of the log through
    quaternion parametrisations of mu and z: the same parameter gradients."""
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(13)
    ns, B = 3, 5
    qm = torch.randn(B, 4, generator=gen, dtype=F64).requires_grad_(True)
    qz = torch.randn(ns, B, 4, generator=gen, dtype=F64).requires_grad_(True)
    gv = torch.randn(ns, B, 3, generator=gen, dtype=F64)
    mu, z = lie_ref.quat_to_mat(qm), lie_ref.quat_to_mat(qz)
    (ref.rel_log(mu, z) * gv).sum().backward()
    want = (qm.grad.clone(), qz.grad.clone())
    qm.grad = qz.grad = None
    gmu, gz = ref.rel_log_vjp(mu.detach(), z.detach(), gv)
    mu, z = lie_ref.quat_to_mat(qm), lie_ref.quat_to_mat(qz)
    ((mu * gmu).sum() + (z * gz).sum()).backward()
    assert (qm.grad - want[0]).abs().max() <= 1e-12 and (qz.grad - want[1]).abs().max() <= 1e-12
    # angle = |rel_log|
    qm.grad = qz.grad = None
    gth = torch.randn(ns, B, generator=gen, dtype=F64)
    mu, z = lie_ref.quat_to_mat(qm), lie_ref.quat_to_mat(qz)
    (ref.rel_log(mu, z).norm(dim=-1) * gth).sum().backward()
    want = (qm.grad.clone(), qz.grad.clone())
    qm.grad = qz.grad = None
    A = mu.detach().expand(ns, B, 3, 3)
    gA, gB = ref.angle_vjp(A, z.detach(), gth)
    mu, z = lie_ref.quat_to_mat(qm), lie_ref.quat_to_mat(qz)
    ((mu * gA.sum(0)).sum() + (z * gB).sum()).backward()
    assert (qm.grad - want[0]).abs().max() <= 1e-12 and (qz.grad - want[1]).abs().max() <= 1e-12
    assert (ref.angle(A, z.detach()) - ref.rel_log(mu, z).norm(dim=-1)).abs().max() <= 1e-15


def test_log_prob_restatement_is_branch_free():
    """log_prob at z = mu exp(v) equals the wrapped density at v, also for |v| in (pi, 2 pi - 0.5):
    the log returns the short way round and the sheets make up for it (k = 10, sigma <= 1)."""
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(14)
    ns, B = 4, 9
    mu = ref.haar(B, gen)
    sigma = 0.2 + 0.8 * torch.rand(B, 3, generator=gen, dtype=F64)
    u = torch.randn(ns, B, 3, generator=gen, dtype=F64)
    u = u / u.norm(dim=-1, keepdim=True)
    for lo, hi in ((0.05, math.pi - 0.1), (math.pi, 2 * math.pi - 0.5)):
        th = lo + (hi - lo) * torch.rand(ns, B, 1, generator=gen, dtype=F64)
        v = u * th
        z = mu @ ref.exp(v)
        got, want = ref.log_prob(mu, z, sigma), lie_ref.so3_log_posterior(v, sigma, 10)
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-11), (got - want).abs().max()


def test_fp32_error_levels_of_the_algorithm():
    """The restatement evaluated in fp32 on the CPU against its fp64 value on the same fp32
    matrix: what the algorithm itself loses in fp32, inside the bounds the GPU tests use
    (1e-5 normwise round trip; 1e-5 |v64| + 1e-6 on v, up to sign at pi; 1e-5 on gR).  The
    reference's own fp32 log_map on the golden matrices is printed beside it."""
    for name in ref.BANDS:
        case = ref.band_case(name)
        R32 = case["R"]
        v32, th32, _ = ref.log_polar(R32)
        assert torch.isfinite(v32).all(), name
        rt, rs = ref.normwise(ref.exp(v32.double()), R32.double())
        dv = (v32.double() - case["v64"]).norm(dim=-1)
        if name in ("near_pi", "half_turn"):
            dv = torch.minimum(dv, (v32.double() + case["v64"]).norm(dim=-1))
        bound = 1e-5 * case["v64"].norm(dim=-1) + 1e-6
        g32 = ref.log_vjp(R32, case["gv"])
        ge, gs = ref.normwise(g32, case["gR64"])
        print(f"{name}: fp32 round trip {float((rt / rs).max()):.2e}, |v - v64| max {float(dv.max()):.2e} "
              f"(bound min {float(bound.min()):.2e}), gR normwise {float((ge / gs).max()):.2e}")
        assert (rt <= 1e-5 * rs).all() and (dv <= bound).all() and torch.isfinite(g32).all()
        if name not in ("near_pi", "half_turn"):
            assert (ge <= 1e-5 * gs).all()
    g = golden("so3_log.npz")
    R, v64 = torch.from_numpy(g["R"]), torch.from_numpy(g["v64"])
    ours = (ref.log_polar(R.float())[0].double() - v64).norm(dim=-1)
    theirs = (torch.from_numpy(g["v32_ref"]).double() - v64).norm(dim=-1)
    print(f"golden, fp32 vs fp64 reference: restatement {float(ours.max()):.2e}, "
          f"reference expression {float(theirs.max()):.2e}")
    assert (ours <= 1e-5 * v64.norm(dim=-1) + 1e-6).all()
