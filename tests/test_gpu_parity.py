"""GPU parity of the HIP path (through the C ABI) against the reference.

Three layers of evidence:
  1. golden vectors produced by the reference code itself (tests/golden, small sizes);
  2. the CPU oracle (oracle/lie_ref.py) on identical seeded inputs at larger sizes;
  3. size-independent properties at full BASELINE sizes (orthogonality, D(b)D(a)=D(ab),
     linearity in F, transpose = inverse).

Tolerance (north_star: "within 1e-5 rel fp32"): graded per sample, normwise —
||y_s - ref_s|| <= 1e-5 ||ref_s|| — because the reference's own fp32 output differs from
its fp64 evaluation elementwise by O(1) relative near zeros.  For
l >= 10 we also require err(HIP vs fp64) <= 2 err(reference fp32 vs fp64).
"""
import glob
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

TOL = 1e-5


def dev(x, device, dtype=None):
    t = torch.as_tensor(np.asarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(device)


def normwise(y, ref):
    y = np.asarray(y, dtype=np.float64).reshape(len(ref), -1)
    r = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    return np.linalg.norm(y - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-30)


def assert_normwise(y, ref, tol=TOL, what=""):
    e = normwise(y, ref)
    assert np.isfinite(e).all(), what
    assert e.max() <= tol, f"{what}: max per-sample rel err {e.max():.3e} > {tol:.1e}"


def assert_parity_fp64(y, ref32, ref64, tol=TOL, what=""):
    """Per sample: within tol of the reference's fp32 output, or no further from the
    fp64 evaluation than 2x the reference's own worst fp32 error on the batch (SURVEY.md
    §8(c) 2x rule; near beta = 0 / pi the fp32 Euler extraction is ill-conditioned and a
    1-ulp difference anywhere upstream moves D by ~1e-5, so the reference's own fp32
    error sets the noise floor).  Also the batch as a whole: ||y - ref64|| <= 2 ||ref32 -
    ref64|| + tol-scaled slack."""
    e32 = normwise(y, ref32)
    e64 = normwise(y, ref64)
    eref = normwise(ref32, ref64)
    floor = 2 * max(eref.max(), 1e-7)
    ok = (e32 <= tol) | (e64 <= floor)
    assert np.isfinite(e32).all(), what
    assert ok.all(), (f"{what}: {np.count_nonzero(~ok)} samples fail; worst e32 {e32.max():.3e}, "
                      f"worst e64 {e64.max():.3e} vs floor {floor:.3e}")
    tot = lambda a, b: np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)  # noqa
    assert tot(y, ref64) <= 2 * tot(ref32, ref64) + 1e-7, what


def host(t):
    return t.detach().cpu().numpy()


def grad_run(fn, inputs, gout, device, dtypes=None):
    xs = [dev(x, device, None if dtypes is None else dtypes[i]).requires_grad_(True)
          for i, x in enumerate(inputs)]
    y = fn(*xs)
    (y * dev(gout, device, y.dtype)).sum().backward()
    return host(y), [host(x.grad) for x in xs]


# ------------------------------------------------------------- conversions
def test_conversions(gpu_device):
    import lie_vae.lie_tools as lt
    g = golden("conversions.npz")
    d = gpu_device
    for tag in ("", "_small", "_large"):
        y, (gv,) = grad_run(lt.rodrigues, [g[f"exp_v{tag}"]], g[f"exp_gR{tag}"], d)
        assert_normwise(y, g[f"exp_R{tag}"], what=f"rodrigues{tag}")
        assert_normwise(gv, g[f"exp_gv{tag}"], 1e-4, what=f"rodrigues grad{tag}")
    assert np.isnan(host(lt.rodrigues(torch.zeros(1, 3, device=d)))).all()

    q = host(lt.group_matrix_to_quaternions(dev(g["haar_R"], d)))
    assert_normwise(q, g["haar_q"], what="mat->quat")
    q = host(lt.group_matrix_to_quaternions(dev(g["gen_R"], d)))
    assert_normwise(q, g["gen_q"], what="mat->quat generic")
    y, (gr,) = grad_run(lt.group_matrix_to_eazyz, [g["haar_R"]], g["haar_gang"], d)
    assert_normwise(y, g["haar_ang"], what="mat->eazyz")
    assert_normwise(gr, g["haar_gR"], 1e-4, what="mat->eazyz grad")
    _, (gr,) = grad_run(lt.group_matrix_to_quaternions, [g["gen_R"]], g["haar_gq"], d)
    assert_normwise(gr, g["gen_gR"], 1e-4, what="mat->quat grad")
    y, (gq,) = grad_run(lt.quaternions_to_eazyz, [g["q_unit"]], g["haar_gang"], d)
    assert_normwise(y, g["q_eazyz"], what="quat->eazyz")
    assert_normwise(gq, g["q_geazyz"], 1e-4, what="quat->eazyz grad")
    y, (gq,) = grad_run(lt.quaternions_to_group_matrix, [g["q_in"]], g["q_gmat"], d)
    assert_normwise(y, g["q_mat"], what="quat->mat")
    assert_normwise(gq, g["q_gq"], 1e-4, what="quat->mat grad")
    y, (ga, gc) = grad_run(lt.s2s1rodrigues, [g["s2s1_axis"], g["s2s1_cs"]], g["s2s1_gR"], d)
    assert_normwise(y, g["s2s1_R"], what="s2s1")
    assert_normwise(ga, g["s2s1_gaxis"], 1e-4, what="s2s1 grad axis")
    assert_normwise(gc, g["s2s1_gcs"], 1e-4, what="s2s1 grad cs")
    y, (g1, g2) = grad_run(lt.s2s2_gram_schmidt, [g["s2s2_v1"], g["s2s2_v2"]], g["s2s2_gR"], d)
    assert_normwise(y, g["s2s2_R"], 1e-12, what="s2s2 fp64")
    assert_normwise(g1, g["s2s2_gv1"], 1e-10, what="s2s2 grad v1")
    assert_normwise(g2, g["s2s2_gv2"], 1e-10, what="s2s2 grad v2")
    # edge rotations (identity, gimbal z-rotations, pi rotations): exact case choice
    q = host(lt.group_matrix_to_quaternions(dev(g["edge_R"], d)))
    np.testing.assert_allclose(q, g["edge_q"], rtol=1e-6, atol=1e-6)
    ang = host(lt.group_matrix_to_eazyz(dev(g["edge_R"], d)))
    np.testing.assert_allclose(ang, g["edge_ang"], rtol=1e-5, atol=1e-5)


def test_empty_batches(gpu_device):
    import lie_vae.lie_tools as lt
    assert lt.rodrigues(torch.zeros(0, 3, device=gpu_device)).shape == (0, 3, 3)
    out = lt.block_wigner_matrix_multiply(torch.zeros(0, 3, device=gpu_device),
                                          torch.zeros(16, 4, device=gpu_device).expand(0, -1, -1), 3)
    assert out.shape == (0, 16, 4)


def test_fused_operator_empty_and_single_sample(gpu_device):
    """The product's operator (torch.ops.lievae.fused_exp_action) at n = 0 -- empty output,
    a zero spectrum gradient -- and n = 1 (one partial sample group) against the modular
    path, forward and backward."""
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    L, C = 10, 10
    M = (L + 1) ** 2
    F = torch.randn(M, C, device=gpu_device, requires_grad=True)
    v = torch.zeros(0, 3, device=gpu_device, requires_grad=True)
    out = ops.fused_exp_action(None, v, F, L)
    assert out.shape == (0, M, C)
    out.backward(torch.zeros(0, M, C, device=gpu_device))
    assert F.grad is not None and torch.count_nonzero(F.grad) == 0 and v.grad.shape == (0, 3)
    F.grad = None
    torch.manual_seed(5)
    v1 = torch.randn(1, 3, device=gpu_device, requires_grad=True)
    out = ops.fused_exp_action(None, v1, F, L)
    g = torch.randn_like(out)
    out.backward(g)
    v2 = v1.detach().clone().requires_grad_(True)
    F2 = F.detach().clone().requires_grad_(True)
    ref = lt.block_wigner_matrix_multiply(lt.group_matrix_to_eazyz(lt.rodrigues(v2)), F2.expand(1, -1, -1), L)
    ref.backward(g)
    assert_normwise(host(out.detach()), host(ref.detach()), tol=1e-5, what="n=1 out")
    assert_normwise(host(F.grad)[None], host(F2.grad)[None], tol=1e-4, what="n=1 gF")
    assert_normwise(host(v1.grad), host(v2.grad), tol=1e-3, what="n=1 gv")


def test_bad_sizes_raise(gpu_device):
    import lie_vae.lie_tools as lt
    from lie_vae._lib import LieVaeHipError
    a = torch.zeros(4, 3, device=gpu_device)
    with pytest.raises(LieVaeHipError, match="l_max"):
        lt.block_wigner_matrix_multiply(a, torch.zeros(4, 22 * 22, 2, device=gpu_device), 21)
    with pytest.raises(LieVaeHipError, match="C must be"):
        lt.block_wigner_matrix_multiply(a, torch.zeros(4, 16, 65, device=gpu_device), 3)


# ------------------------------------------------------------------ Wigner-D
def test_wigner_blocks_vs_golden(gpu_device):
    import lie_vae.lie_tools as lt
    g = golden("wigner.npz")
    for l in range(11):
        D = host(lt.wigner_d_matrix(dev(g["ang"], gpu_device), l))
        assert_normwise(D, g[f"D{l}"], what=f"D{l}")
    D = host(lt.wigner_d_matrix(dev(g["ang20"], gpu_device), 20))
    assert_normwise(D, g["D20"], what="D20")


@pytest.mark.parametrize("l", [0, 1, 2, 5, 10, 20])
def test_wigner_properties(gpu_device, l):
    """Reference property tests (lie_tools.py:337-357) on the HIP output."""
    import lie_vae.lie_tools as lt
    torch.manual_seed(l)
    ra = lt.random_group_matrices(2000, device=gpu_device)
    rb = lt.random_group_matrices(2000, device=gpu_device)
    wa = lt.wigner_d_matrix(lt.group_matrix_to_eazyz(ra), l)
    wb = lt.wigner_d_matrix(lt.group_matrix_to_eazyz(rb), l)
    wc = lt.wigner_d_matrix(lt.group_matrix_to_eazyz(ra.bmm(rb)), l)
    eye = torch.eye(2 * l + 1, device=gpu_device).expand_as(wa)
    torch.testing.assert_close(wa @ wa.transpose(-2, -1), eye, rtol=1e-4, atol=1e-5)
    winv = lt.wigner_d_matrix(lt.group_matrix_to_eazyz(ra.transpose(1, 2).contiguous()), l)
    torch.testing.assert_close(wa @ winv, eye, rtol=1e-4, atol=1e-5)
    # the reference bound (1e-3, checked there for l <= 5); Euler extraction in fp32 is
    # ill-conditioned near beta = 0, and D's sensitivity to angle error grows ~l
    tol = 1e-3 * max(1.0, l / 5)
    torch.testing.assert_close(wb.bmm(wa), wc, rtol=tol, atol=tol)


# ----------------------------------------------------------------- the action
ACTION_FILES = sorted(glob.glob(os.path.join(GOLDEN, "action_*.npz")))


def parse_case(name):
    return [int(x[1:]) for x in name[:-4].split("_")[1:]]


@pytest.mark.parametrize("path", ACTION_FILES, ids=[os.path.basename(p) for p in ACTION_FILES])
def test_action_vs_golden(gpu_device, path):
    import lie_vae.lie_tools as lt
    name = os.path.basename(path)
    L, C, t, p = parse_case(name)
    g = golden(name)
    n = g["ang"].shape[0]

    def f(a, s):
        sx = s if p else s.expand(n, -1, -1)
        return lt.block_wigner_matrix_multiply(a, sx, L, transpose=bool(t))

    y, (ga, gs) = grad_run(f, [g["ang"], g["spec"]], g["gout"], gpu_device)
    assert_normwise(y, g["out"], what=f"{name} out")
    if "out64" in g:
        e_hip = normwise(y, g["out64"])
        e_ref = normwise(g["out"], g["out64"])
        assert e_hip.max() <= 2 * max(e_ref.max(), 1e-7), (e_hip.max(), e_ref.max())
    assert_normwise(ga, g["gang"], 1e-4, what=f"{name} dangles")
    if p:
        assert_normwise(gs, g["gspec"], 1e-4, what=f"{name} dspectrum")
    else:
        assert_normwise(gs[None], g["gspec"][None], 1e-5, what=f"{name} dspectrum")


@pytest.mark.parametrize("L,C,n,transpose", [(10, 10, 4096, False), (3, 10, 256, False),
                                             (10, 10, 1000, True), (20, 10, 512, False),
                                             (7, 64, 300, False), (5, 1, 777, False),
                                             (15, 13, 257, True)])
def test_action_vs_oracle(gpu_device, L, C, n, transpose):
    """Seeded Haar angles at BASELINE size (config 2: B=4096, l=10, C=10) and ragged
    sizes, against the CPU oracle on the same fp32 inputs."""
    import lie_vae.lie_tools as lt
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(1234 + L + n)
    q = torch.randn(n, 4, generator=gen)
    ang = lie_ref.mat_to_eazyz(lie_ref.quat_to_mat(q))
    spec = torch.randn((L + 1) ** 2, C, generator=gen)
    ref = lie_ref.block_wigner_apply(ang, spec.expand(n, -1, -1), L, transpose)
    out = lt.block_wigner_matrix_multiply(ang.to(gpu_device), spec.to(gpu_device).expand(n, -1, -1),
                                          L, transpose)
    assert_normwise(host(out), ref.numpy(), what=f"L{L} C{C} n{n}")


def test_action_linearity_and_transpose(gpu_device):
    """Size-independent properties at 65536 samples: linear in F; D^T D F = F."""
    import lie_vae.lie_tools as lt
    torch.manual_seed(5)
    n, L, C = 65536, 10, 10
    ang = lt.group_matrix_to_eazyz(lt.random_group_matrices(n, device=gpu_device))
    f1 = torch.randn((L + 1) ** 2, C, device=gpu_device)
    f2 = torch.randn((L + 1) ** 2, C, device=gpu_device)
    o1 = lt.block_wigner_matrix_multiply(ang, f1.expand(n, -1, -1), L)
    o2 = lt.block_wigner_matrix_multiply(ang, f2.expand(n, -1, -1), L)
    o12 = lt.block_wigner_matrix_multiply(ang, (2 * f1 - f2).expand(n, -1, -1), L)
    assert_normwise(host(o12), host(2 * o1 - o2), 1e-5, what="linearity")
    back = lt.block_wigner_matrix_multiply(ang, o1, L, transpose=True)
    assert_normwise(host(back), host(f1.expand(n, -1, -1)), 2e-5, what="D^T D F = F")
    # norm preservation per degree block (D orthogonal)
    torch.testing.assert_close(o1.norm(dim=(1, 2)), f1.norm().expand(n), rtol=1e-5, atol=0)


def test_action_bf16_output(gpu_device):
    import lie_vae._ops as ops
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(99)
    n, L, C = 2048, 20, 10
    ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n))
    spec = torch.randn((L + 1) ** 2, C, generator=gen)
    out = ops.group_action(ang.to(gpu_device), spec.to(gpu_device), L, out_dtype=torch.bfloat16)
    # every row, including the ragged last group (2048 = 341 * 6 + 2)
    ref = lie_ref.block_wigner_apply(ang, spec.expand(n, -1, -1), L)
    assert out.dtype == torch.bfloat16
    assert_normwise(host(out.float()), ref.numpy(), 4e-3, what="bf16 out")
    y = host(out.float()).reshape(n, -1)
    r = ref.numpy().reshape(n, -1)
    err = np.linalg.norm(y - r, axis=1) / np.linalg.norm(r, axis=1)
    assert err.max() <= 4e-3, f"bf16 out: worst row {err.argmax()} rel err {err.max():.2e}"


# --------------------------------------------------------------- fused path
def test_fused_vs_golden(gpu_device):
    import lie_vae._ops as ops
    g = golden("fused_exp_action.npz")
    d = gpu_device
    out = ops.fused_exp_action(dev(g["mu"], d), dev(g["v"], d), dev(g["item_rep"], d), 10)
    assert_normwise(host(out).reshape(len(g["out"]), -1), g["out"], what="fused")


def test_fused_matches_modular_and_grads(gpu_device):
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    torch.manual_seed(3)
    n, L, C = 4096, 10, 10
    mu = lt.random_group_matrices(n, device=gpu_device)
    v = torch.randn(n, 3, device=gpu_device) * 0.5
    F = torch.randn((L + 1) ** 2, C, device=gpu_device)
    gout = torch.randn(n, (L + 1) ** 2, C, device=gpu_device)
    xs = [t.clone().requires_grad_(True) for t in (mu, v, F)]
    y1 = ops.fused_exp_action(*xs, L)
    (y1 * gout).sum().backward()
    ys = [t.clone().requires_grad_(True) for t in (mu, v, F)]
    z = ops.so3_sample(ys[0], ys[1][None])[0]
    y2 = lt.block_wigner_matrix_multiply(lt.group_matrix_to_eazyz(z), ys[2].expand(n, -1, -1), L)
    (y2 * gout).sum().backward()
    from oracle import lie_ref
    mu_c, v_c, F_c = mu.cpu(), v.cpu(), F.cpu()
    ref32 = lie_ref.block_wigner_apply(lie_ref.mat_to_eazyz(lie_ref.so3_sample(mu_c, v_c)),
                                       F_c.expand(n, -1, -1), L)
    ref64 = lie_ref.block_wigner_apply(
        lie_ref.mat_to_eazyz(lie_ref.so3_sample(mu_c.double(), v_c.double())),
        F_c.double().expand(n, -1, -1), L)
    assert_parity_fp64(host(y1), ref32.numpy(), ref64.numpy(), what="fused (mu) vs oracle")
    assert_parity_fp64(host(y2), ref32.numpy(), ref64.numpy(), what="modular vs oracle")
    assert_normwise(host(xs[2].grad)[None], host(ys[2].grad)[None], 1e-4, what="grad F")
    # mu / v: the fused backward against the oracle's fp64 autograd, not against the modular
    # path -- that one differentiates the fp32 extraction at the fp32 acos angles, which near
    # beta = 0 / pi is off by ~1e-3 of a sample's gradient, while the fused path saves an
    # accurate beta and runs its VJP in fp64 (tests/test_gpu_action_matrix.py)
    gout_c = gout.cpu()
    gF64, (gmu64, gv64) = _oracle_grads(mu_c, v_c, None, F_c, gout_c, L, False)
    _, (gmu32, gv32) = _oracle_grads(mu_c, v_c, None, F_c, gout_c, L, False, torch.float32)
    assert_normwise(host(xs[2].grad)[None], gF64[None], 1e-5, what="grad F vs oracle")
    assert_grad_parity(host(xs[0].grad), gmu32, gmu64, what="grad mu")
    assert_grad_parity(host(xs[1].grad), gv32, gv64, what="grad v")


def test_action_bwd_reproducible_and_looped(gpu_device):
    """lv_group_action_bwd (backward tile kernel + dF slab reduce) is bitwise reproducible
    (no atomics), agrees with the oracle's autograd, and its grid-capped path -- blocks
    looping over several sample groups, more than 4096 groups -- matches 4096-sample
    chunks to fp32 summation-order noise (the degree segments, hence the order in which a
    sample's angle-gradient partials are added, depend on the batch size)."""
    import lie_vae._ops as ops
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(11)
    for L, n, transpose, shared in [(10, 4099, False, True), (10, 777, True, True),
                                    (3, 1001, False, False), (12, 300, False, True)]:
        ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n))
        M = (L + 1) ** 2
        F = torch.randn(M, 10, generator=gen) if shared else torch.randn(n, M, 10, generator=gen)
        gout = torch.randn(n, M, 10, generator=gen)
        grads = []
        for _ in range(2):
            a = ang.to(gpu_device).requires_grad_(True)
            f = F.to(gpu_device).requires_grad_(True)
            (ops.group_action(a, f, L, transpose=transpose) * gout.to(gpu_device)).sum().backward()
            grads.append((host(a.grad), host(f.grad)))
        assert np.array_equal(grads[0][0], grads[1][0]) and np.array_equal(grads[0][1], grads[1][1]), \
            ("not reproducible", L, n, transpose, shared)
        m = min(n, 300)
        a64 = ang[:m].double().requires_grad_(True)
        f64 = (F if shared else F[:m]).double().requires_grad_(True)
        fe = f64.expand(m, -1, -1) if shared else f64
        (lie_ref.block_wigner_apply(a64, fe, L, transpose=transpose) * gout[:m].double()).sum().backward()
        assert_normwise(grads[0][0][:m], a64.grad.numpy(), 1e-4, what=f"gang L={L}")
        if not shared:
            assert_normwise(grads[0][1][:m].reshape(m, -1), f64.grad.numpy().reshape(m, -1), 1e-4,
                            what=f"gF L={L}")
    # looped path: 50,000 samples = 8,334 groups > the 4,096-block cap
    L, n = 10, 50000
    ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n)).to(gpu_device)
    F = torch.randn((L + 1) ** 2, 10, generator=gen).to(gpu_device)
    gout = torch.randn(n, (L + 1) ** 2, 10, generator=gen).to(gpu_device)
    a = ang.clone().requires_grad_(True)
    f = F.clone().requires_grad_(True)
    (ops.group_action(a, f, L) * gout).sum().backward()
    ga_parts, gf_sum = [], torch.zeros_like(F, dtype=torch.float64)
    for lo in range(0, n, 4096):
        ap = ang[lo:lo + 4096].clone().requires_grad_(True)
        fp = F.clone().requires_grad_(True)
        (ops.group_action(ap, fp, L) * gout[lo:lo + 4096]).sum().backward()
        ga_parts.append(ap.grad)
        gf_sum += fp.grad.double()
    # one plan (persistent, 8,334 groups) vs 4,096-sample chunks (683 blocks): the
    # same per-sample sums in different orders (column tree, degree split over waves)
    assert_normwise(host(a.grad), host(torch.cat(ga_parts)), 1e-4, what="looped angle grads")
    assert_normwise(host(f.grad)[None], gf_sum.cpu().numpy()[None], 1e-5, what="looped dF")


def test_action_bwd_persistent_kernel(gpu_device):
    """The persistent backward (action_bwd_persist.h: 3 blocks per CU walk the 6-sample
    groups, the next group's multiples prefetched, one dF slab per block; plan mode 3 from
    CUs + 1 groups at l <= 10, C = 10, shared spectrum) at ragged large batches: bitwise
    reproducible run to run; angle gradients and dF against chunks of one group per CU
    (the one-group kernel) at fp32 summation-order noise; the oracle's fp64 autograd on a
    sample of the batch; transposed."""
    import lie_vae._lib as lib
    import lie_vae._ops as ops
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(31)
    L, C = 10, 10
    M = (L + 1) ** 2
    pb = 3 * lib.load().lv_compute_units()  # 768 on MI355X
    for n, transpose in [(6 * (pb + 1) + 5, False), (65536, False), (30001, True)]:
        p = lib.plan("bwd", n, L, C, 1)
        assert p["tile"] == 3 and p["blocks"] == min(pb, -(-n // 6)), p
        ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n)).to(gpu_device)
        F = torch.randn(M, C, generator=gen).to(gpu_device)
        gout = torch.randn(n, M, C, generator=gen).to(gpu_device)
        grads = []
        for _ in range(2):
            a = ang.clone().requires_grad_(True)
            f = F.clone().requires_grad_(True)
            (ops.group_action(a, f, L, transpose=transpose) * gout).sum().backward()
            grads.append((a.grad.clone(), f.grad.clone()))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]), \
            ("persistent backward not reproducible", n)
        ga_parts, gf_sum = [], torch.zeros_like(F, dtype=torch.float64)
        ch = 6 * lib.load().lv_compute_units()  # one group per CU: the one-group kernel
        for lo in range(0, n, ch):
            assert lib.plan("bwd", min(ch, n - lo), L, C, 1)["tile"] == 1
            ap = ang[lo:lo + ch].clone().requires_grad_(True)
            fp = F.clone().requires_grad_(True)
            (ops.group_action(ap, fp, L, transpose=transpose) * gout[lo:lo + ch]).sum().backward()
            ga_parts.append(ap.grad)
            gf_sum += fp.grad.double()
        # per-sample angle gradients are sums of ~4,000 chain terms with cancellation; the
        # chunks' plans (a ragged last chunk runs 8 degree sets) add them in another order:
        # the suite's gradient tolerance
        assert_normwise(host(grads[0][0]), host(torch.cat(ga_parts)), 1e-4,
                        what=f"persistent angle grads n={n}")
        assert_normwise(host(grads[0][1])[None], gf_sum.cpu().numpy()[None], 1e-5,
                        what=f"persistent dF n={n}")
        m = 256
        idx = torch.randperm(n, generator=gen)[:m]
        a64 = ang[idx].cpu().double().requires_grad_(True)
        f64 = F.cpu().double().requires_grad_(True)
        (lie_ref.block_wigner_apply(a64, f64.expand(m, -1, -1), L, transpose=transpose)
         * gout[idx].cpu().double()).sum().backward()
        assert_normwise(host(grads[0][0][idx.to(gpu_device)]), a64.grad.numpy(), 1e-4,
                        what=f"persistent gang vs oracle n={n}")


def _oracle_grads(mu, v, ang, F, gout, L, transpose, dtype=torch.float64, chunk=4096):
    """The oracle's autograd (fp64, or fp32 for the reference's own error floor) over the
    whole batch, 4,096 samples at a time: dF (the batch reduction of item_rep.expand's
    gradient, decoders.py:53 backward through lie_tools.py:226-253) summed over the chunks
    in fp64, so host time stays bounded and the mathematics is unchanged.  With mu / v
    given, the fused path's chain z = mu @ exp(v) -> ZYZ -> D(z)·F
    (reparameterize.py:269-273, lie_tools.py:178) is differentiated to (gmu, gv); else
    angles -> D·F to gang."""
    from oracle import lie_ref
    n = gout.shape[0]
    gF = torch.zeros(F.shape, dtype=torch.float64)
    g_in = []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        g = gout[lo:hi].to(dtype)
        f = F.detach().to(dtype).clone().requires_grad_(True)
        if v is not None:
            m_ = mu[lo:hi].detach().to(dtype).clone().requires_grad_(True)
            v_ = v[lo:hi].detach().to(dtype).clone().requires_grad_(True)
            a = lie_ref.mat_to_eazyz(lie_ref.so3_sample(m_, v_))
            (lie_ref.block_wigner_apply(a, f.expand(hi - lo, -1, -1), L, transpose) * g).sum().backward()
            g_in.append((m_.grad, v_.grad))
        else:
            a_ = ang[lo:hi].detach().to(dtype).clone().requires_grad_(True)
            (lie_ref.block_wigner_apply(a_, f.expand(hi - lo, -1, -1), L, transpose) * g).sum().backward()
            g_in.append((a_.grad,))
        gF += f.grad.double()
    return gF.numpy(), [torch.cat(p).double().numpy().reshape(n, -1) for p in zip(*g_in)]


def assert_grad_parity(y, ref32, ref64, tol=1e-4, what=""):
    """Per-sample input gradients: within tol (normwise) of the oracle's fp64 autograd, or
    no further from it than 2x the reference's own worst fp32 autograd error on the batch
    -- the forward's rule (assert_parity_fp64): near beta = 0 / pi the ZYZ
    gradients scale like 1/sin(beta) and the fp32 reference itself is off by up to ~6e-4
    there (65,536 Haar samples).  The batch as a whole: within max(tol, 2x the reference's
    batch error)."""
    y = np.asarray(y, np.float64).reshape(len(ref64), -1)
    e_hip, e_ref = normwise(y, ref64), normwise(ref32, ref64)
    ok = (e_hip <= tol) | (e_hip <= 2 * e_ref.max())
    assert np.isfinite(e_hip).all(), what
    assert ok.all(), (f"{what}: {np.count_nonzero(~ok)} samples fail; worst {e_hip.max():.3e} "
                      f"(reference fp32 worst {e_ref.max():.3e})")
    tot = lambda a: np.linalg.norm(a - ref64) / np.linalg.norm(ref64)  # noqa: E731
    assert tot(y) <= max(tol, 2 * tot(ref32)), (what, tot(y), tot(ref32))


@pytest.mark.parametrize("n,transpose", [(1536, False), (4096, False), (65536, False), (30001, True)])
def test_shared_spectrum_grads_vs_oracle_fp64(gpu_device, n, transpose):
    """The shared-spectrum gradient dF and the fused path's (gmu, gv) against the oracle's
    fp64 autograd over the WHOLE batch, at the sizes where the one-group kernel + reduce5
    (1,536 = one group per CU: plan mode 1) and the persistent kernel (4,096 with one group
    per block, 65,536 and 30,001 transposed walking the groups: plan mode 3) produce them.  The other backward tests compare these kernels with each other
    (HIP chunks) or with the oracle on a few hundred samples; here the full reduction is
    pinned.  Tolerances: dF 1e-5 normwise over the (M, C) matrix; angle / v / mu
    gradients per sample 1e-4 normwise or the 2x rule against the reference's own fp32
    autograd (assert_grad_parity)."""
    import lie_vae._lib as lib
    import lie_vae._ops as ops
    from oracle import lie_ref
    L, C = 10, 10
    M = (L + 1) ** 2
    assert lib.plan("bwd", n, L, C, 1)["tile"] == (1 if -(-n // 6) <= lib.load().lv_compute_units() else 3)
    torch.manual_seed(4242 + n)  # haar_matrices draws from the global generator
    gen = torch.Generator().manual_seed(4242 + n)
    mu = lie_ref.haar_matrices(n)
    v = torch.randn(n, 3, generator=gen) * 0.5
    ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n))
    F = torch.randn(M, C, generator=gen)
    gout = torch.randn(n, M, C, generator=gen)
    d = gpu_device
    g_d = gout.to(d)
    # modular: lv_group_action_bwd
    a = ang.to(d).requires_grad_(True)
    f = F.to(d).requires_grad_(True)
    (ops.group_action(a, f, L, transpose=transpose) * g_d).sum().backward()
    gF64, (gang64,) = _oracle_grads(None, None, ang, F, gout, L, transpose)
    _, (gang32,) = _oracle_grads(None, None, ang, F, gout, L, transpose, torch.float32)
    assert_normwise(host(f.grad)[None], gF64[None], 1e-5, what=f"dF n={n}")
    assert_grad_parity(host(a.grad), gang32, gang64, what=f"gang n={n}")
    # fused training path: lv_fused_exp_action_bwd (VJP beside the reduce)
    xs = [t.to(d).requires_grad_(True) for t in (mu, v, F)]
    (ops.fused_exp_action(*xs, L, transpose=transpose) * g_d).sum().backward()
    gFf64, (gmu64, gv64) = _oracle_grads(mu, v, None, F, gout, L, transpose)
    _, (gmu32, gv32) = _oracle_grads(mu, v, None, F, gout, L, transpose, torch.float32)
    assert_normwise(host(xs[2].grad)[None], gFf64[None], 1e-5, what=f"fused dF n={n}")
    assert_grad_parity(host(xs[1].grad), gv32, gv64, what=f"fused gv n={n}")
    assert_grad_parity(host(xs[0].grad), gmu32, gmu64, what=f"fused gmu n={n}")


_PERSIST_GRID_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import lie_vae._lib as lib
import lie_vae._ops as ops
d = np.load(sys.argv[2])
dev = torch.device("cuda:0")
ang = torch.from_numpy(d["ang"]).to(dev).requires_grad_(True)
F = torch.from_numpy(d["F"]).to(dev).requires_grad_(True)
gout = torch.from_numpy(d["gout"]).to(dev)
p = lib.plan("bwd", ang.shape[0], 10, 10, 1)
(ops.group_action(ang, F, 10) * gout).sum().backward()
np.savez(sys.argv[3], ga=ang.grad.cpu().numpy(), gf=F.grad.cpu().numpy(), blocks=p["blocks"], tile=p["tile"])
"""


def test_persistent_backward_other_grid_sizes_vs_oracle(gpu_device, tmp_path):
    """The persistent backward's grid is sized from the device's CU count (3 blocks per CU,
    lv_compute_units), so a smaller part (a CPX partition) runs more groups per block and
    another dF summation order.  With the A/B library's LV_BWD_PERSIST_BPC (blocks per CU)
    the same kernel runs 1 and 2 blocks per CU on this device (256 / 512 blocks at 30,001
    samples): dF and the angle gradients against the oracle's fp64 autograd, as the
    product grid is (test_shared_spectrum_grads_vs_oracle_fp64)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    from oracle import lie_ref
    n, L, C = 30001, 10, 10
    torch.manual_seed(77)
    gen = torch.Generator().manual_seed(77)
    ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n))
    F = torch.randn((L + 1) ** 2, C, generator=gen)
    gout = torch.randn(n, (L + 1) ** 2, C, generator=gen)
    inp = str(tmp_path / "in.npz")
    np.savez(inp, ang=ang.numpy(), F=F.numpy(), gout=gout.numpy())
    gF64, (ga64,) = _oracle_grads(None, None, ang, F, gout, L, False)
    _, (ga32,) = _oracle_grads(None, None, ang, F, gout, L, False, torch.float32)
    import lie_vae._lib as lib
    cus = lib.load().lv_compute_units()
    for bpc in (1, 2):
        out = str(tmp_path / f"g{bpc}.npz")
        env = dict(os.environ, LV_BWD_PERSIST_BPC=str(bpc),
                   LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", "liblievae_hip_ab.so"))
        subprocess.run([sys.executable, "-c", _PERSIST_GRID_SCRIPT, pkg, inp, out], env=env, check=True,
                       timeout=180)
        r = np.load(out)
        assert int(r["tile"]) == 3 and int(r["blocks"]) == bpc * cus, (bpc, int(r["blocks"]))
        assert_normwise(r["gf"][None], gF64[None], 1e-5, what=f"dF, {bpc} blocks per CU")
        assert_grad_parity(r["ga"], ga32, ga64, what=f"gang, {bpc} blocks per CU")


_FWD_SEG_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import lie_vae._ops as ops
dev = torch.device("cuda:0")
out = {}
for n in (4097, 16385):
    g = torch.Generator().manual_seed(n)
    v = torch.randn(n, 3, generator=g).to(dev)
    F = torch.randn(121, 10, generator=g).to(dev)
    out[f"y{n}"] = ops.fused_exp_action(None, v, F, 10).cpu().numpy()
import lie_vae._lib as lib
out["seg"] = lib.plan("fwd", 1, 0, lib.LV_DTYPE_F32, 4097, 10, 10)["segments"]
np.savez(sys.argv[2], **out)
"""


def test_forward_wave_counts_and_degree_sets_bitwise(gpu_device, tmp_path):
    """The forward tile kernel's plan (waves per block by groups per CU, degree sets by the
    cost model) changes which wave computes which degree, never a degree's arithmetic:
    every wave count 4-8 and a hand-made degree set (A/B library knobs LV_TILE_NSEG /
    LV_TILE_MASKS) give the product library's output bit for bit (config-2 shape, a ragged
    4,097 and 16,385)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    runs = {"product": {}}
    for k in (4, 5, 6, 7, 8):
        runs[f"nseg{k}"] = {"LV_TILE_NSEG": str(k)}
    runs["masks"] = {"LV_TILE_NSEG": "6", "LV_TILE_MASKS": "400:200:102:84:48:31"}
    res = {}
    for tag, extra in runs.items():
        out = str(tmp_path / f"{tag}.npz")
        # the ctypes path (no liblievae_torch.so, which links the product library), so the
        # A/B library's kernels are the ones that run
        env = dict(os.environ, LIEVAE_TORCH_OPS_LIB=str(tmp_path / "none.so"), **extra)
        if tag != "product":
            env["LIEVAE_HIP_LIB"] = os.path.join(pkg, "lie_vae", "liblievae_hip_ab.so")
        subprocess.run([sys.executable, "-c", _FWD_SEG_SCRIPT, pkg, out], env=env, check=True, timeout=180)
        res[tag] = np.load(out)
    for k in (4, 5, 6, 7, 8):
        assert int(res[f"nseg{k}"]["seg"]) == k  # the knob took effect
    for tag, r in res.items():
        for key in ("y4097", "y16385"):
            assert np.array_equal(r[key], res["product"][key]), (tag, key)


def test_action_large_tiles_fallback_vs_oracle(gpu_device):
    """Tiles too large for the LDS plans (large C at high l; include/lievae.h plan mode 2):
    the forward's grid-stride kernel and the backward's global-spectrum fallback (dF slab
    in the workspace), and a per-sample spectrum at l = 20, C = 64 (LDS budget raised),
    against the oracle's autograd."""
    import lie_vae._lib as lib
    import lie_vae._ops as ops
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(12)
    for L, C, n, shared in [(20, 16, 97, True), (15, 64, 61, True), (20, 64, 13, False)]:
        mode = lib.plan("bwd", n, L, C, int(shared))["tile"]
        assert mode == (2 if shared else 0), (L, C, mode)
        M = (L + 1) ** 2
        ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n))
        F = torch.randn(M, C, generator=gen) if shared else torch.randn(n, M, C, generator=gen)
        gout = torch.randn(n, M, C, generator=gen)
        a = ang.to(gpu_device).requires_grad_(True)
        f = F.to(gpu_device).requires_grad_(True)
        y = ops.group_action(a, f, L)
        (y * gout.to(gpu_device)).sum().backward()
        a64 = ang.double().requires_grad_(True)
        f64 = F.double().requires_grad_(True)
        fe = f64.expand(n, -1, -1) if shared else f64
        y64 = lie_ref.block_wigner_apply(a64, fe, L)
        (y64 * gout.double()).sum().backward()
        assert_normwise(host(y).reshape(n, -1), y64.detach().numpy().reshape(n, -1), 1e-5,
                        what=f"y L={L} C={C}")
        assert_normwise(host(a.grad), a64.grad.numpy(), 1e-4, what=f"gang L={L} C={C}")
        assert_normwise(host(f.grad).reshape(-1, M * C), f64.grad.numpy().reshape(-1, M * C),
                        1e-4, what=f"gF L={L} C={C}")


_FGLOBAL_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import lie_vae._ops as ops
L, n = 10, 4099
g = torch.Generator().manual_seed(13)
ang = (torch.rand(n, 3, generator=g) * 6 - 3).cuda().requires_grad_(True)
F = torch.randn((L + 1) ** 2, 10, generator=g).cuda().requires_grad_(True)
gout = torch.randn(n, (L + 1) ** 2, 10, generator=g).cuda()
(ops.group_action(ang, F, L) * gout).sum().backward()
np.savez(sys.argv[2], ga=ang.grad.cpu().numpy(), gf=F.grad.cpu().numpy())
"""


def test_action_bwd_global_spectrum_mode_bitwise(gpu_device, tmp_path):
    """The fallback mode (spectrum from global memory, dF slab accumulated in the block's
    workspace row) keeps the LDS mode's summation order: forced on for the config-2 shape
    (LV_BWD_FGLOBAL=1, read once per process, hence a child process), the gradients are
    bitwise those of the LDS mode for the same segment plan (LV_BWD_NSEG=2 in both: the
    LDS mode's default at this shape is the persistent kernel, switched off here with
    LV_BWD_PERSIST_MIN=0, and then the 4-segment 3-waves-per-SIMD plan).  The knobs
    exist only in the A/B build of the same kernels (liblievae_hip_ab.so, -DLV_AB_KNOBS);
    the product library ignores the environment (test_product_library_ignores_knobs)."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    outs = []
    for forced in ("0", "1"):
        path = str(tmp_path / f"g{forced}.npz")
        env = dict(os.environ, LV_BWD_FGLOBAL=forced, LV_BWD_NSEG="2", LV_BWD_PERSIST_MIN="0",
                   LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", "liblievae_hip_ab.so"))
        subprocess.run([sys.executable, "-c", _FGLOBAL_SCRIPT, pkg, path], env=env, check=True,
                       timeout=180)
        outs.append(np.load(path))
    assert np.array_equal(outs[0]["ga"], outs[1]["ga"])
    assert np.array_equal(outs[0]["gf"], outs[1]["gf"])


_BWD_AB_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import lie_vae._lib as lib
from lie_vae._lib import call, ptr, stream
dev = torch.device("cuda:0")
L, C = 10, 10
M = (L + 1) ** 2
out = {}
for tag, n, transpose in (("one", 777, 1), ("persist", 6 * (lib.load().lv_compute_units() + 1) + 5, 0)):
    g = torch.Generator().manual_seed(n)
    ang = (torch.rand(n, 3, generator=g) * 6 - 3).to(dev)
    v = torch.randn(n, 3, generator=g).to(dev)
    F = torch.randn(M, C, generator=g).to(dev)
    gout = torch.randn(n, M, C, generator=g).to(dev)
    q = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))[0]
    mu = (q * torch.linalg.det(q)[:, None, None]).contiguous().to(dev)  # rotations (det +1)
    p = lib.plan("bwd", n, L, C, 1)
    ws_bytes = lib.load().lv_group_action_bwd_workspace(n, L, C, 1)
    ws = torch.empty(max(ws_bytes, 1), device=dev, dtype=torch.uint8)
    gang, gF = torch.empty_like(ang), torch.empty_like(F)
    call("lv_group_action_bwd", ptr(ang), ptr(F), 0, ptr(gout), ptr(gang), ptr(gF), n, L, C, transpose,
         ptr(ws), ws_bytes, stream())
    gmu, gv, gF2 = torch.empty_like(mu), torch.empty_like(v), torch.empty_like(F)
    call("lv_fused_exp_action_bwd", ptr(mu), ptr(v), ptr(ang), ptr(F), ptr(gout), ptr(gmu), ptr(gv), ptr(gF2),
         n, L, C, transpose, ptr(ws), ws_bytes, stream())
    for k, t in (("mu", mu), ("gang", gang), ("gF", gF), ("gmu", gmu), ("gv", gv), ("gF2", gF2)):
        out[f"{tag}_{k}"] = t.cpu().numpy()
    out[f"{tag}_plan"] = np.array([p["tile"], p["segments"]])
np.savez(sys.argv[2], **out)
"""


def test_action_bwd_ab_library_without_knobs_matches_product_bitwise(gpu_device, tmp_path):
    """The A/B library (-DLV_AB_KNOBS) is a separate build of the backward's source: with no
    knob set it gives the product library's gradients bit for bit -- lv_group_action_bwd and
    lv_fused_exp_action_bwd with a mean, at l = 10, C = 10 for the one-group kernel (777
    samples, transposed: 8 degree sets) and the persistent kernel (one group more than a
    block per CU, ragged).  One child process per library, on the ctypes path."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    res = {}
    for tag, name in (("product", "liblievae_hip.so"), ("ab", "liblievae_hip_ab.so")):
        path = str(tmp_path / f"{tag}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith(("LV_BWD_", "LV_SEG_", "LV_STAMPS"))}
        env.update(LIEVAE_TORCH_OPS_LIB=str(tmp_path / "none.so"),
                   LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", name))
        subprocess.run([sys.executable, "-c", _BWD_AB_SCRIPT, pkg, path], env=env, check=True, timeout=180)
        res[tag] = np.load(path)
    assert list(res["product"]["one_plan"]) == [1, 8] and int(res["product"]["persist_plan"][0]) == 3
    assert sorted(res["ab"].files) == sorted(res["product"].files)
    for key in res["product"].files:
        assert np.array_equal(res["ab"][key], res["product"][key]), key
    for key in ("one_gang", "one_gF", "one_gv", "one_gmu", "persist_gang", "persist_gF", "persist_gv"):
        a = res["product"][key]
        assert np.isfinite(a).all() and np.abs(a).max() > 0, key  # the kernels ran


def test_exp_eazyz_vjp_matches_modular_bitwise(gpu_device):
    """lv_exp_eazyz_vjp (the fused path's prologue backward in one kernel) against the
    three modular kernels it replaces -- so3_exp_fwd / so3_sample_fwd, mat_to_eazyz_bwd,
    so3_exp_bwd / so3_sample_bwd -- with and without a mean rotation.  The chain runs in
    fp64 (in fp32 it is ill-conditioned near beta = 0 / pi, tests/test_gpu_action_matrix.py):
    the fp64 entry gives the fp64 modular kernels' gradients bit for bit, the fp32 entry
    those of its inputs cast up, rounded once to fp32, bit for bit."""
    import lie_vae.lie_tools as lt
    from lie_vae._lib import call, ptr, stream
    torch.manual_seed(5)
    n = 3001
    v = torch.randn(n, 3, device=gpu_device)
    mu = lt.random_group_matrices(n, device=gpu_device).contiguous()
    ga = torch.randn(n, 3, device=gpu_device)

    def modular(m, v, ga, sfx):
        z = torch.empty(n, 3, 3, device=gpu_device, dtype=v.dtype)
        if m is None:
            call("lv_so3_exp_fwd" + sfx, ptr(v), ptr(z), n, stream())
        else:
            call("lv_so3_sample_fwd" + sfx, ptr(m), ptr(v), ptr(z), 1, n, stream())
        gz = torch.empty_like(z)
        call("lv_mat_to_eazyz_bwd" + sfx, ptr(z), ptr(ga), ptr(gz), n, stream())
        gv, gmu = torch.empty_like(v), None
        if m is None:
            call("lv_so3_exp_bwd" + sfx, ptr(v), ptr(gz), ptr(gv), n, stream())
        else:
            gmu = torch.empty_like(m)
            call("lv_so3_sample_bwd" + sfx, ptr(m), ptr(v), ptr(gz), ptr(gmu), ptr(gv), 1, n, stream())
        return gv, gmu

    for m in (None, mu):
        what = "mu" if m is not None else "exp"
        gv1 = torch.empty_like(v)
        gmu1 = torch.empty_like(mu) if m is not None else None
        call("lv_exp_eazyz_vjp", ptr(m), ptr(v), ptr(ga), ptr(gmu1), ptr(gv1), n, stream())
        m64 = m.double() if m is not None else None
        v64, ga64 = v.double(), ga.double()
        gv64 = torch.empty_like(v64)
        gmu64 = torch.empty_like(m64) if m is not None else None
        call("lv_exp_eazyz_vjp_f64", ptr(m64), ptr(v64), ptr(ga64), ptr(gmu64), ptr(gv64), n, stream())
        gv2, gmu2 = modular(m64, v64, ga64, "_f64")
        assert torch.equal(gv64, gv2), what
        assert torch.equal(gv1, gv2.float()), what
        if m is not None:
            assert torch.equal(gmu64, gmu2) and torch.equal(gmu1, gmu2.float())


def test_fused_exp_action_bwd_matches_modular_bitwise(gpu_device):
    """lv_fused_exp_action_bwd (group-action backward with the exp -> ZYZ VJP in the dF
    reduce's launch, action_bwd_reduce5_vjp_kernel, for the one-group and the persistent
    tile kernels) against lv_group_action_bwd + lv_exp_eazyz_vjp, bit for bit: with and
    without a mean, transposed, ragged batches, the persistent kernel (20,003 samples) and
    the large-tile spectrum mode."""
    import lie_vae._lib as lib
    from lie_vae._lib import call, ptr, stream
    import lie_vae.lie_tools as lt
    torch.manual_seed(6)
    for L, C, n, transpose in [(10, 10, 4099, False), (10, 10, 777, True), (6, 3, 50000, False),
                               (20, 16, 301, False), (10, 10, 20003, True)]:
        M = (L + 1) ** 2
        v = torch.randn(n, 3, device=gpu_device)
        mu = lt.random_group_matrices(n, device=gpu_device).contiguous()
        F = torch.randn(M, C, device=gpu_device)
        gout = torch.randn(n, M, C, device=gpu_device)
        ws_bytes = lib.load().lv_group_action_bwd_workspace(n, L, C, 1)
        ws = torch.empty(max(ws_bytes, 1), device=gpu_device, dtype=torch.uint8)
        for m in (None, mu):
            out = torch.empty(n, M, C, device=gpu_device)
            ang = torch.empty(n, 3, device=gpu_device)
            call("lv_fused_exp_action_fwd", ptr(m), ptr(v), ptr(F), 0, ptr(out), 0, ptr(ang), n,
                 L, C, int(transpose), stream())
            gv1, gF1 = torch.empty_like(v), torch.empty_like(F)
            gmu1 = torch.empty_like(mu) if m is not None else None
            call("lv_fused_exp_action_bwd", ptr(m), ptr(v), ptr(ang), ptr(F), ptr(gout),
                 ptr(gmu1), ptr(gv1), ptr(gF1), n, L, C, int(transpose), ptr(ws), ws_bytes,
                 stream())
            gang, gF2 = torch.empty_like(ang), torch.empty_like(F)
            call("lv_group_action_bwd", ptr(ang), ptr(F), 0, ptr(gout), ptr(gang), ptr(gF2), n,
                 L, C, int(transpose), ptr(ws), ws_bytes, stream())
            gv2 = torch.empty_like(v)
            gmu2 = torch.empty_like(mu) if m is not None else None
            call("lv_exp_eazyz_vjp", ptr(m), ptr(v), ptr(gang), ptr(gmu2), ptr(gv2), n, stream())
            what = (L, C, n, transpose, m is not None)
            assert torch.equal(gv1, gv2), what
            assert torch.equal(gF1, gF2), what
            if m is not None:
                assert torch.equal(gmu1, gmu2), what


def test_fused_torch_operator_matches_python_function_bitwise(gpu_device):
    """torch.ops.lievae.fused_exp_action (csrc/torch_ops.cpp, the C++ autograd function the
    product calls) against the Python autograd.Function over the same C ABI: outputs and
    gradients bit for bit, with and without a mean, transposed, bf16 output, fp64 inputs
    (gradients come back in the inputs' dtypes), and under hipGraph capture."""
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    assert ops._TORCH_OPS, "liblievae_torch.so not loaded: the product's operator is missing"
    torch.manual_seed(11)
    for L, C, n, transpose, odt, idt, with_mu in [
            (10, 10, 4096, False, torch.float32, torch.float32, False),
            (10, 10, 1001, True, torch.float32, torch.float32, True),
            (20, 10, 777, False, torch.bfloat16, torch.float32, False),
            (6, 7, 300, False, torch.float32, torch.float64, True)]:
        M = (L + 1) ** 2
        v0 = torch.randn(n, 3, device=gpu_device, dtype=idt)
        F0 = torch.randn(M, C, device=gpu_device, dtype=idt)
        mu0 = lt.random_group_matrices(n, device=gpu_device).to(idt).contiguous() if with_mu else None
        gout = torch.randn(n, M, C, device=gpu_device, dtype=odt)
        res = []
        for use_op in (True, False):
            v, F = v0.clone().requires_grad_(True), F0.clone().requires_grad_(True)
            mu = mu0.clone().requires_grad_(True) if with_mu else None
            if use_op:
                out = torch.ops.lievae.fused_exp_action(mu, v, F, L, transpose, odt == torch.bfloat16)
            else:
                out = ops._FusedExpAction.apply(mu, v, ops._f32c(F), L, transpose, odt)
            out.backward(gout)
            res.append((out, v.grad, F.grad, mu.grad if with_mu else None))
        what = (L, C, n, transpose, odt, idt, with_mu)
        (o1, gv1, gF1, gm1), (o2, gv2, gF2, gm2) = res
        assert o1.dtype == odt and gv1.dtype == idt and gF1.dtype == idt, what
        assert torch.equal(o1, o2), what
        assert torch.equal(gv1, gv2.to(idt)), what
        assert torch.equal(gF1, gF2.to(idt)), what
        if with_mu:
            assert gm1.dtype == idt and torch.equal(gm1, gm2.to(idt)), what
    # the operator under graph capture (fresh workspace from the capture pool)
    n, L, C = 4096, 10, 10
    v = torch.randn(n, 3, device=gpu_device, requires_grad=True)
    F = torch.randn((L + 1) ** 2, C, device=gpu_device, requires_grad=True)
    gout = torch.randn(n, (L + 1) ** 2, C, device=gpu_device)
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        out = torch.ops.lievae.fused_exp_action(None, v, F, L, False, False)
        out.backward(gout)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    ref = (out.detach().clone(), v.grad.clone(), F.grad.clone())
    v.grad = None
    F.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = torch.ops.lievae.fused_exp_action(None, v, F, L, False, False)
        out_g.backward(gout)
    g.replay()
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(out_g, ref[0]) and torch.equal(v.grad, ref[1]) and torch.equal(F.grad, ref[2])


def test_torch_operator_refuses_cpu_or_mixed_inputs(gpu_device):
    """the operator INTEGRATION.md tells integrators to call directly
    checks every input's device before any launch -- a CPU mean (or v / spectrum) raises a
    clean RuntimeError instead of reaching the kernel as an invalid device pointer -- and
    the Python entry point refuses an out_dtype the kernels cannot write."""
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    assert ops._TORCH_OPS
    n, L, C = 64, 3, 4
    v = torch.randn(n, 3, device=gpu_device)
    F = torch.randn((L + 1) ** 2, C, device=gpu_device)
    mu = lt.random_group_matrices(n, device=gpu_device).contiguous()
    for args in [(mu.cpu(), v, F), (mu, v.cpu(), F), (mu, v, F.cpu()), (None, v, F.cpu())]:
        with pytest.raises(RuntimeError, match="device tensors only|one device"):
            torch.ops.lievae.fused_exp_action(*args, L, False, False)
        with pytest.raises(RuntimeError, match="CPU"):
            ops.fused_exp_action(*args, L)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.fused_exp_action(mu, v, F, L, out_dtype=torch.float16)
    # the device stays usable after the refusals
    out = torch.ops.lievae.fused_exp_action(mu, v, F, L, False, False)
    torch.cuda.synchronize(gpu_device)
    assert torch.isfinite(out).all()


def test_fused_vs_oracle_config2(gpu_device):
    """Config 2 exactly: B=4096, l=10, C=10, v ~ N(0,1), shared F (no mu)."""
    import lie_vae._ops as ops
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(0)
    n, L, C = 4096, 10, 10
    v = torch.randn(n, 3, generator=gen)
    F = torch.randn((L + 1) ** 2, C, generator=gen)
    ref = lie_ref.block_wigner_apply(lie_ref.mat_to_eazyz(lie_ref.so3_exp(v)),
                                     F.expand(n, -1, -1), L)
    ref64 = lie_ref.block_wigner_apply(lie_ref.mat_to_eazyz(lie_ref.so3_exp(v.double())),
                                       F.double().expand(n, -1, -1), L)
    out = ops.fused_exp_action(None, v.to(gpu_device), F.to(gpu_device), L)
    assert_parity_fp64(host(out), ref.numpy(), ref64.numpy(), what="config2 fused")


# ---------------------------------------------------------------- reparam
@pytest.mark.parametrize("mode", ["alg", "s2s2", "q", "s2s1"])
def test_so3_reparam_vs_golden(gpu_device, mode):
    import lie_vae.reparameterize as rp
    g = golden("reparam.npz")
    mean_cls = {"alg": rp.AlgebraMean, "s2s2": rp.S2S2Mean, "q": rp.QuaternionMean,
                "s2s1": rp.S2S1Mean}[mode]
    rep = rp.SO3reparameterize(rp.N0reparameterize(10, z_dim=3), mean_cls(10), k=10)
    with torch.no_grad():
        for name, p in rep.named_parameters():
            p.copy_(torch.from_numpy(g[f"{mode}_p_{name}"]))
    rep = rep.to(gpu_device)
    h = dev(g[f"{mode}_h"], gpu_device).requires_grad_(True)
    eps = dev(g[f"{mode}_eps"], gpu_device)
    z = rep(h, 2, eps=eps)
    assert_normwise(host(rep.mu_lie), g[f"{mode}_mu"], what="mu")
    assert_normwise(host(rep.v).reshape(-1, 3), g[f"{mode}_v"].reshape(-1, 3), what="v")
    assert_normwise(host(z).reshape(-1, 9), g[f"{mode}_z"].reshape(-1, 9), what="z")
    lp = host(rep.log_posterior())
    np.testing.assert_allclose(lp, g[f"{mode}_logpost"], rtol=1e-5, atol=1e-4)
    kl = rep.kl()
    # the reference's prior is a float64 tensor (reparameterize.py:265-267): kl follows it
    assert kl.dtype == torch.float64 and g[f"{mode}_kl"].dtype == np.float64, kl.dtype
    np.testing.assert_allclose(host(kl), g[f"{mode}_kl"], rtol=1e-5, atol=1e-4)
    ((z * dev(g[f"{mode}_gz"], gpu_device)).sum() +
     (kl * dev(g[f"{mode}_gk"], gpu_device)).sum()).backward()
    assert_normwise(host(h.grad)[None], g[f"{mode}_gh"][None], 1e-4, what="dh")
    for name, p in rep.named_parameters():
        assert_normwise(host(p.grad)[None], g[f"{mode}_g_{name}"][None], 1e-4, what=f"d{name}")


def test_log_posterior_wide_range(gpu_device):
    import lie_vae._ops as ops
    g = golden("reparam.npz")
    v = dev(g["lp_v"], gpu_device).requires_grad_(True)
    s = dev(g["lp_sigma"], gpu_device).requires_grad_(True)
    lp = ops.so3_log_posterior(v, s, 10)
    np.testing.assert_allclose(host(lp), g["lp_out"], rtol=1e-5, atol=1e-4)
    (lp * dev(g["lp_g"], gpu_device)).sum().backward()
    assert_normwise(host(v.grad).reshape(-1, 3), g["lp_gv"].reshape(-1, 3), 1e-4, what="gv")
    assert_normwise(host(s.grad)[None], g["lp_gsigma"][None], 1e-4, what="gsigma")


# ------------------------------------------------------------- toy dataset (§8 f4)
def test_toy_dataset_generate(gpu_device):
    """ToyDataset.generate (datasets.py:143-158) on the GPU vs the oracle applied to the
    same poses and spectrum; ragged last chunk (n not a multiple of batch_size)."""
    from lie_vae.experiments.datasets import ToyDataset
    from oracle import lie_ref
    ds = ToyDataset.generate(n=150, degrees=6, rep_copies=10, device=gpu_device,
                             batch_size=64)
    q, h, x = (host(t) for t in ds.tensors)
    assert q.shape == (150, 4) and h.shape == (150, 49, 10) and x.shape == (150, 49, 10)
    np.testing.assert_allclose(np.linalg.norm(h[0]), 10.0, rtol=1e-6)
    qt = torch.from_numpy(q)
    ref = lie_ref.block_wigner_apply(lie_ref.quat_to_eazyz(qt),
                                     torch.from_numpy(h[0]).expand(150, -1, -1), 6)
    ref64 = lie_ref.block_wigner_apply(lie_ref.quat_to_eazyz(qt.double()),
                                       torch.from_numpy(h[0]).double().expand(150, -1, -1), 6)
    assert_parity_fp64(x, ref.numpy(), ref64.numpy(), what="toy generate")
    # norm preserved per sample and column: D is orthogonal
    np.testing.assert_allclose(np.linalg.norm(x, axis=1), np.linalg.norm(h, axis=1),
                               rtol=1e-5)


def test_c10_specialised_tile_kernel_bitwise(gpu_device):
    """The tile kernel is compiled twice: specialised for C = 10 (ActionNet's default
    rep_copies; row-major spectrum staging, immediate offsets) and generic in C
    (column-major staging).  Columns are independent and both chains round identically,
    so C = 10 must agree bit for bit with the first 10 columns of C = 11 (fused and angle
    inputs, ragged last group, transpose, bf16 output) -- and with the non-tile kernel
    that a per-sample spectrum takes."""
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    DEV = gpu_device
    for L, n, transpose, bf16 in [(10, 4099, False, False), (10, 4096, True, False),
                                  (3, 1000, False, False), (12, 777, False, True),
                                  (20, 301, False, False)]:
        gen = torch.Generator().manual_seed(7 + L + n)
        v = torch.randn(n, 3, generator=gen).to(DEV)
        F11 = torch.randn((L + 1) ** 2, 11, generator=gen).to(DEV)
        F10 = F11[:, :10].contiguous()
        od = torch.bfloat16 if bf16 else torch.float32
        a = ops.fused_exp_action(None, v, F10, L, transpose=transpose, out_dtype=od)
        b = ops.fused_exp_action(None, v, F11, L, transpose=transpose, out_dtype=od)
        assert torch.equal(a, b[..., :10]), ("fused", L, n, transpose, bf16)
        ang = lt.group_matrix_to_eazyz(lt.rodrigues(v))
        a = ops.group_action(ang, F10, L, transpose=transpose, out_dtype=od)
        b = ops.group_action(ang, F11, L, transpose=transpose, out_dtype=od)
        assert torch.equal(a, b[..., :10]), ("angles", L, n, transpose, bf16)
        if not bf16:  # per-sample spectrum: the register-multiples, row-pair-store kernel
            c = ops.group_action(ang, F10.expand(n, -1, -1).contiguous(), L, transpose=transpose)
            assert torch.equal(a, c), ("per-sample", L, n, transpose)


# ------------------------------------------------ end to end: VAE glue + IWAE (a11-a16, f3)
def _vae_oracle(vae, x, eps, L, k=10):
    """The toy-mode VAE pipeline restated with oracle functions on the CPU (vae.py:113-204,
    reparameterize.py:100-278, decoders.py:47-56): returns x_recon (n,B,M,C), the
    summed-squares recon loss (n,B), log q(z|x) (n,B) and kl (B,)."""
    from oracle import lie_ref
    rep = vae.rep_group
    with torch.no_grad():
        h = vae.encoder(x)
        mu = lie_ref.so3_exp(rep.mean_module.map(h))
        sig = lie_ref.n0_sigma(rep.reparameterize.sigma_linear(h))
        v = lie_ref.n0_sample(sig, eps)
        z = lie_ref.so3_sample(mu, v)
        n, B = eps.shape[:2]
        ang = lie_ref.mat_to_eazyz(z.reshape(-1, 3, 3))
        xr = lie_ref.action_decode(ang, vae.decoder.item_rep, L).reshape(n, B, *x.shape[1:])
        recon = ((xr - x) ** 2).sum(-1).sum(-1)
        lq = lie_ref.so3_log_posterior(v, sig, k)
        kl = (lq + math.log(8 * math.pi ** 2)).mean(0)
    return xr, recon, lq, kl


def test_vae_toy_elbo_and_log_likelihood_vs_oracle(gpu_device):
    """Toy-mode VAE (MLP encoder, SO(3) latent with AlgebraMean, ActionNet l = 6, C = 10,
    no deconv): ELBO terms with injected eps, and the importance-weighted log-likelihood
    (vae.py:164-171) with the device RNG replayed, against the oracle pipeline."""
    from lie_vae.experiments.vae import VAE
    L, B, n = 6, 16, 5
    torch.manual_seed(3)
    vae = VAE(latent_mode='so3', decoder_mode='action', degrees=L, encode_mode='toy',
              deconv_mode='toy', rep_copies=10, mean_mode='alg')
    x = torch.randn(B, (L + 1) ** 2, 10)
    eps = torch.randn(n, B, 3)
    xr_ref, recon_ref, lq_ref, kl_ref = _vae_oracle(vae, x, eps, L)
    vg = VAE(latent_mode='so3', decoder_mode='action', degrees=L, encode_mode='toy',
             deconv_mode='toy', rep_copies=10, mean_mode='alg')
    vg.load_state_dict(vae.state_dict())
    vg = vg.to(gpu_device)
    xg = x.to(gpu_device)
    with torch.no_grad():
        recon, kl_sum, _ = vg.elbo(xg, n, eps=eps.to(gpu_device))
        xr = vg.forward(xg, n, eps=eps.to(gpu_device))
    assert_normwise(host(xr).reshape(n * B, -1), xr_ref.numpy().reshape(n * B, -1), 1e-5,
                    what="x_recon")
    np.testing.assert_allclose(host(recon), recon_ref.numpy(), rtol=1e-4)
    np.testing.assert_allclose(host(kl_sum), kl_ref.numpy(), rtol=1e-4, atol=1e-4)
    assert kl_sum.dtype == torch.float64  # the reference's float64 prior (reparameterize.py:265-267)
    # IWAE: log_likelihood draws eps with torch.randn on the device; replay the same draw
    torch.cuda.manual_seed(11)
    eps2 = torch.randn((n, B, 3), device=gpu_device)
    torch.cuda.manual_seed(11)
    with torch.no_grad():
        ll = vg.log_likelihood(xg, n)
    assert ll.dtype == torch.float64
    _, recon2, lq2, _ = _vae_oracle(vae, x, eps2.cpu(), L)
    w = -recon2 - math.log(8 * math.pi ** 2) - lq2
    ll_ref = (torch.logsumexp(w, 0) - math.log(n)).mean()
    np.testing.assert_allclose(float(ll), float(ll_ref), rtol=1e-4)


# ---------------------------------------------------------------- fp64 inputs (a2-a6)
def test_fp64_maps_follow_input_dtype(gpu_device):
    """The reference's per-sample maps return the input dtype (lie_tools.py:28-38,61:
    v.new_tensor, eye(dtype=v.dtype)) and its self-tests run them in fp64
    (lie_tools.py:271-291).  fp64 in -> the *_f64 kernels: fp64 out, within 1e-12 of the
    oracle's fp64 restatement, gradients within 1e-10 of its autograd; the reference's
    own log/exp round-trip self-test (test_log_exp, lie_tools.py:280-291) in fp64."""
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    from oracle import lie_ref
    torch.manual_seed(21)
    n = 2000
    f64 = torch.float64
    v = torch.randn(n, 3, dtype=f64) * 1.3
    q = lie_ref.haar_quaternions(n, dtype=f64)
    r = lie_ref.quat_to_mat(q)
    ax = torch.nn.functional.normalize(torch.randn(n, 3, dtype=f64), dim=-1)
    th = torch.rand(n, dtype=f64) * 6.0
    cs = torch.stack((torch.cos(th), torch.sin(th)), -1)
    mu = lie_ref.haar_matrices(n, dtype=f64)
    cases = [
        ("rodrigues", lambda x: lt.rodrigues(x[0]), lambda x: lie_ref.so3_exp(x[0]), [v]),
        ("quat_to_mat", lambda x: lt.quaternions_to_group_matrix(x[0]),
         lambda x: lie_ref.quat_to_mat(x[0]), [q]),
        ("mat_to_quat", lambda x: lt.group_matrix_to_quaternions(x[0]),
         lambda x: lie_ref.mat_to_quat(x[0]), [r]),
        ("quat_to_eazyz", lambda x: lt.quaternions_to_eazyz(x[0]),
         lambda x: lie_ref.quat_to_eazyz(x[0]), [q]),
        ("mat_to_eazyz", lambda x: lt.group_matrix_to_eazyz(x[0]),
         lambda x: lie_ref.mat_to_eazyz(x[0]), [r]),
        ("s2s1", lambda x: lt.s2s1rodrigues(x[0], x[1]), lambda x: lie_ref.s2s1_exp(x[0], x[1]),
         [ax, cs]),
        ("so3_sample", lambda x: ops.so3_sample(x[0], x[1][None])[0],
         lambda x: lie_ref.so3_sample(x[0], x[1]), [mu, v]),
    ]
    for name, f, ref, xs in cases:
        xg = [t.to(gpu_device).requires_grad_(True) for t in xs]
        y = f(xg)
        assert y.dtype == f64, (name, y.dtype)
        xc = [t.clone().requires_grad_(True) for t in xs]
        yr = ref(xc)
        err = (host(y) - yr.detach().numpy())
        scale = np.abs(yr.detach().numpy()).max()
        # Euler extraction is ill-conditioned near beta = 0: a 1-ulp change of q moves the
        # angles by far more than 1 ulp, so those maps get a looser (still fp64) bound
        tol = 1e-9 if "eazyz" in name else 1e-12
        assert np.abs(err).max() <= tol * max(scale, 1.0), (name, np.abs(err).max())
        g = torch.randn(yr.shape, dtype=f64)
        (y * g.to(gpu_device)).sum().backward()
        (yr * g).sum().backward()
        for a, b in zip(xg, xc):
            assert a.grad.dtype == f64
            ga, gb = host(a.grad), b.grad.numpy()
            assert np.abs(ga - gb).max() <= (1e-7 if "eazyz" in name else 1e-10) * \
                max(np.abs(gb).max(), 1.0), (name, np.abs(ga - gb).max())
    # the reference's own self-test, fp64: rodrigues / log_map round trip at its
    # tolerances (test_log_exp(0.1, 1E-6), test_log_exp(10, 1E-6), lie_tools.py:442-443)
    for scale, tol in ((0.1, 1e-6), (10.0, 1e-6)):
        vs = torch.randn(50, 3, dtype=f64, device=gpu_device) * scale
        for k in range(50):
            R = lt.rodrigues(vs[k])
            w = lt.map_to_lie_vector(lt.log_map(R))
            R2 = lt.rodrigues(w)
            np.testing.assert_allclose(host(R2), host(R), rtol=tol, atol=tol)
