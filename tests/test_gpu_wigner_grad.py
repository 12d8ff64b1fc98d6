"""wigner_d_matrix on the GPU: the one-degree forward (lv_wigner_d_block_fwd) and the angle
gradients of the block and packed forms (lv_wigner_d_block_bwd, lv_wigner_d_bwd).

The reference everywhere is oracle.lie_ref.wigner_d under fp64 autograd on the CPU, fed the
fp32 angles cast up.  Gradients are graded per sample, normwise, at 1e-4 -- the bound the
group action's angle gradient already carries (test_gpu_parity.py); on these inputs the
oracle's own fp32 autograd is within 9.3e-6 of its fp64 autograd."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_FWD = 1e-5
TOL_GRAD = 1e-4
SPECIAL = [(0.0, 0.0, 0.0), (0.3, math.pi, -0.2), (3.0, 1e-3, -3.0)]


def host(t):
    return t.detach().cpu().numpy()


def normwise(y, ref):
    y = np.asarray(y, dtype=np.float64).reshape(len(ref), -1)
    r = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    return np.linalg.norm(y - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-30)


def assert_normwise(y, ref, tol, what):
    e = normwise(y, ref)
    assert np.isfinite(e).all(), what
    assert e.max() <= tol, f"{what}: max per-sample rel err {e.max():.3e} > {tol:.1e}"
    return e.max()


def make_angles(n, seed):
    """alpha, gamma uniform in (-pi, pi), beta uniform in (0, pi); rows 0..2 the special
    triples (identity, beta = pi, beta near 0 with |alpha|, |gamma| near pi)."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 3, generator=gen)
    a = torch.stack([(2 * u[:, 0] - 1) * math.pi, u[:, 1] * math.pi, (2 * u[:, 2] - 1) * math.pi], 1)
    for i, row in enumerate(SPECIAL[:n]):
        a[i] = torch.tensor(row)
    return a


def oracle_grad(ang32, loss_fn):
    """fp64 autograd on the CPU of loss_fn(angles) at the fp32 angles cast up."""
    a = ang32.detach().cpu().double().requires_grad_(True)
    loss_fn(a).backward()
    return a.grad.numpy()


def block_grad(ang, G, l, device):
    import lie_vae.lie_tools as lt
    a = ang.to(device).requires_grad_(True)
    (lt.wigner_d_matrix(a, l) * G.to(device)).sum().backward()
    return host(a.grad)


@pytest.mark.parametrize("l", range(21))
def test_block_forward_equals_packed_block_and_oracle(gpu_device, l):
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    from oracle import lie_ref
    n, nn = 37, 2 * l + 1
    ang = make_angles(n, 300 + l)
    a = ang.to(gpu_device)
    D = lt.wigner_d_matrix(a, l)
    assert D.shape == (n, nn, nn) and D.dtype == torch.float32 and not D.requires_grad
    packed = ops.wigner_blocks(a, l)
    off = l * (2 * l - 1) * (2 * l + 1) // 3
    assert packed.shape == (n, off + nn * nn)
    assert torch.equal(D, packed[:, off:].reshape(n, nn, nn)), "block forward != packed block"
    assert_normwise(host(D), lie_ref.wigner_d(ang, l).numpy(), TOL_FWD, f"D_{l}")


@pytest.mark.parametrize("l", range(21))
def test_block_gradient_vs_oracle(gpu_device, l):
    """Measured worst per-sample normwise error on MI355X, l = 0..20: see the table in
    DESIGN.md (Wigner-D blocks); the bound is 1e-4 for every l."""
    import lie_vae.lie_tools as lt
    from oracle import lie_ref
    n, nn = 67, 2 * l + 1
    ang = make_angles(n, 400 + l)
    G = torch.randn(n, nn, nn, generator=torch.Generator().manual_seed(500 + l))
    a = ang.to(gpu_device).requires_grad_(True)
    D = lt.wigner_d_matrix(a, l)
    assert D.requires_grad
    (D * G.to(gpu_device)).sum().backward()
    got = host(a.grad)
    assert got.shape == (n, 3) and got.dtype == np.float32
    if l == 0:
        assert np.array_equal(got, np.zeros_like(got))
        print("wigner grad l=0: exactly zero")
        return
    want = oracle_grad(ang, lambda x: (lie_ref.wigner_d(x, l) * G.double()).sum())
    e = normwise(got, want)
    print(f"wigner grad l={l}: worst per-sample normwise error {e.max():.3e}")
    assert np.isfinite(e).all() and e.max() <= TOL_GRAD, (l, e.max())


@pytest.mark.parametrize("l", [1, 6, 20])
def test_gradient_independent_of_batch_and_deterministic(gpu_device, l):
    """n (2l+1) is no multiple of the 256-thread block and spans several blocks; a sample's
    gradient is bitwise the same in two runs, and alone as a batch of one."""
    import lie_vae.lie_tools as lt
    nn = 2 * l + 1
    n = 67 if l > 1 else 200
    # forward: 256 (sample, column) threads per block; backward: whole samples per block
    assert (n * nn) % 256 != 0 and n * nn > 2 * 256 and n > 2 * min(256 // nn, 64)
    ang = make_angles(n, 600 + l)
    G = torch.randn(n, nn, nn, generator=torch.Generator().manual_seed(700 + l))
    g1 = block_grad(ang, G, l, gpu_device)
    g2 = block_grad(ang, G, l, gpu_device)
    assert np.array_equal(g1, g2), "not reproducible"
    for i in (0, 1, n - 2, n - 1):
        alone = block_grad(ang[i:i + 1], G[i:i + 1], l, gpu_device)
        assert alone.shape == (1, 3)
        assert np.array_equal(alone[0], g1[i]), (l, i, alone[0], g1[i])
    a0 = torch.zeros(0, 3, device=gpu_device, requires_grad=True)
    D0 = lt.wigner_d_matrix(a0, l)
    assert D0.shape == (0, nn, nn)
    D0.sum().backward()
    assert a0.grad.shape == (0, 3)


def test_gradient_shapes_and_layouts(gpu_device):
    import lie_vae.lie_tools as lt
    from oracle import lie_ref
    l, nn = 3, 7
    gen = torch.Generator().manual_seed(800)

    # leading batch dimensions
    ang = make_angles(30, 801).reshape(2, 3, 5, 3)
    G = torch.randn(2, 3, 5, nn, nn, generator=gen)
    a = ang.to(gpu_device).requires_grad_(True)
    D = lt.wigner_d_matrix(a, l)
    assert D.shape == (2, 3, 5, nn, nn)
    (D * G.to(gpu_device)).sum().backward()
    assert a.grad.shape == (2, 3, 5, 3)
    want = oracle_grad(ang, lambda x: (lie_ref.wigner_d(x, l) * G.double()).sum())
    assert_normwise(host(a.grad).reshape(30, 3), want.reshape(30, 3), TOL_GRAD, "leading dims")

    # a transposed view of D: the upstream gradient arrives non-contiguous
    n = 19
    ang = make_angles(n, 802)
    G = torch.randn(n, nn, nn, generator=gen)
    a = ang.to(gpu_device).requires_grad_(True)
    (lt.wigner_d_matrix(a, l).transpose(-1, -2) * G.to(gpu_device)).sum().backward()
    want = oracle_grad(ang, lambda x: (lie_ref.wigner_d(x, l).transpose(-1, -2) * G.double()).sum())
    assert_normwise(host(a.grad), want, TOL_GRAD, "transposed upstream")

    # D used twice: the two upstream gradients are accumulated
    G2 = torch.randn(n, nn, nn, generator=gen)
    a = ang.to(gpu_device).requires_grad_(True)
    D = lt.wigner_d_matrix(a, l)
    ((D * G.to(gpu_device)).sum() + (D * D * G2.to(gpu_device)).sum()).backward()

    def twice(x):
        d = lie_ref.wigner_d(x, l)
        return (d * G.double()).sum() + (d * d * G2.double()).sum()
    assert_normwise(host(a.grad), oracle_grad(ang, twice), TOL_GRAD, "D used twice")

    # angles as a non-contiguous slice of an (n, 4) tensor
    base = torch.cat([torch.randn(n, 1, generator=gen), ang], 1)
    b = base.to(gpu_device).requires_grad_(True)
    sl = b[:, 1:]
    assert not sl.is_contiguous()
    (lt.wigner_d_matrix(sl, l) * G.to(gpu_device)).sum().backward()
    want = oracle_grad(ang, lambda x: (lie_ref.wigner_d(x, l) * G.double()).sum())
    assert_normwise(host(b.grad)[:, 1:], want, TOL_GRAD, "sliced angles")
    assert np.array_equal(host(b.grad)[:, 0], np.zeros(n, dtype=np.float32))

    # fp64 angles: computed in fp32 (on the angles rounded to fp32), returned in fp64
    a32 = ang.to(gpu_device).requires_grad_(True)
    (lt.wigner_d_matrix(a32, l) * G.to(gpu_device)).sum().backward()
    a64 = ang.double().to(gpu_device).requires_grad_(True)
    D64 = lt.wigner_d_matrix(a64, l)
    assert D64.dtype == torch.float32
    (D64 * G.to(gpu_device)).sum().backward()
    assert a64.grad.dtype == torch.float64
    assert torch.equal(a64.grad, a32.grad.double())
    assert_normwise(host(a64.grad), want, TOL_GRAD, "fp64 angles")


@pytest.mark.parametrize("L", [4, 12])
def test_packed_blocks_gradient(gpu_device, L):
    import lie_vae._ops as ops
    from oracle import lie_ref
    n = 33
    tot = (L + 1) * (2 * L + 1) * (2 * L + 3) // 3
    ang = make_angles(n, 900 + L)
    G = torch.randn(n, tot, generator=torch.Generator().manual_seed(950 + L))
    grads = []
    for _ in range(2):
        a = ang.to(gpu_device).requires_grad_(True)
        D = ops.wigner_blocks(a, L)
        assert D.shape == (n, tot) and D.requires_grad
        (D * G.to(gpu_device)).sum().backward()
        grads.append(host(a.grad))
    assert np.array_equal(grads[0], grads[1]), "not reproducible"

    def packed(x):
        tot_loss, off = 0.0, 0
        for l in range(L + 1):
            nn = 2 * l + 1
            tot_loss = tot_loss + (lie_ref.wigner_d(x, l) * G[:, off:off + nn * nn].reshape(n, nn, nn).double()).sum()
            off += nn * nn
        return tot_loss
    assert_normwise(grads[0], oracle_grad(ang, packed), TOL_GRAD, f"packed L={L}")


def test_gradient_consistent_with_action_kernels(gpu_device):
    """The group action's angle gradient against the hand-rolled D.bmm(F) through
    wigner_d_matrix, per-sample spectrum, same upstream."""
    import lie_vae.lie_tools as lt
    from oracle import lie_ref
    L, C, n = 3, 2, 50
    M = (L + 1) ** 2
    gen = torch.Generator().manual_seed(1000)
    ang = make_angles(n, 1001)
    F = torch.randn(n, M, C, generator=gen)
    gout = torch.randn(n, M, C, generator=gen)
    Fd, gd = F.to(gpu_device), gout.to(gpu_device)

    a = ang.to(gpu_device).requires_grad_(True)
    (lt.block_wigner_matrix_multiply(a, Fd, L) * gd).sum().backward()
    g_action = host(a.grad)

    a = ang.to(gpu_device).requires_grad_(True)
    out = torch.cat([lt.wigner_d_matrix(a, l).bmm(Fd[:, l * l:(l + 1) ** 2, :]) for l in range(L + 1)], 1)
    (out * gd).sum().backward()
    g_rolled = host(a.grad)

    want = oracle_grad(ang, lambda x: (lie_ref.block_wigner_apply(x, F.double(), L) * gout.double()).sum())
    assert_normwise(g_rolled, g_action, TOL_GRAD, "hand-rolled vs action kernels")
    assert_normwise(g_action, want, TOL_GRAD, "action kernels vs oracle")
    assert_normwise(g_rolled, want, TOL_GRAD, "hand-rolled vs oracle")
