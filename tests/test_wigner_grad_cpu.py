"""CPU checks of the differentiable Wigner-D entry points (lv_wigner_d_block_fwd / _bwd,
lv_wigner_d_bwd): exports, argument checks ahead of any launch, the no-CPU-fallback rule,
and the derivative convention the VJP kernel rests on, pinned against the oracle's fp64
autograd."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

NEW = ("lv_wigner_d_block_fwd", "lv_wigner_d_block_bwd", "lv_wigner_d_bwd")


def test_wigner_grad_exports():
    from lie_vae import _lib
    text = open(os.path.join(REPO, "include", "lievae.h")).read()
    header = set(re.findall(r"\b(lv_\w+)\s*\(", text))
    lib = _lib.load()
    for name in NEW:
        assert name in header, name
        assert name in _lib.EXPORTED, name
        assert hasattr(lib, name), name
    assert lib.lv_abi_version() == 1  # additive change


def test_wigner_grad_argument_checks_before_any_launch():
    """Dummy non-null pointers, no device: every refusal comes back as LV_ERR_ARG (-1) with
    a message before anything is launched or dereferenced; an empty batch is a no-op."""
    from lie_vae import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(16)  # never dereferenced: the checks run first
    fwd, bwd, pbwd = lib.lv_wigner_d_block_fwd, lib.lv_wigner_d_block_bwd, lib.lv_wigner_d_bwd

    def refused(rc, word):
        msg = lib.lv_last_error()
        assert rc == -1 and msg and word in msg, (rc, msg)

    for l in (-1, 21):
        refused(fwd(P, P, 4, l, None), b"must be in [0, 20]")
        refused(bwd(P, P, P, 4, l, None), b"must be in [0, 20]")
        refused(pbwd(P, P, P, 4, l, None), b"must be in [0, 20]")
    refused(fwd(None, P, 4, 3, None), b"null")
    refused(fwd(P, None, 4, 3, None), b"null")
    for f in (bwd, pbwd):
        refused(f(None, P, P, 4, 3, None), b"null")
        refused(f(P, None, P, 4, 3, None), b"null")   # gD
        refused(f(P, P, None, 4, 3, None), b"null")   # gang
        refused(f(P, P, P, -1, 3, None), b"n must be >= 0")
    refused(fwd(P, P, -1, 3, None), b"n must be >= 0")
    # a grid past 2^31 - 1 blocks: forward one thread per (sample, column), 256 per block;
    # backward whole samples per block (floor(256 / (2l+1)), at most 64)
    for l in (0, 3, 20):
        nn = 2 * l + 1
        nmax_f = (2 ** 31 - 1) * 256 // nn
        nmax_b = (2 ** 31 - 1) * min(256 // nn, 64)
        refused(fwd(P, P, nmax_f + 1, l, None), b"too large")
        refused(bwd(P, P, P, nmax_b + 1, l, None), b"too large")
        refused(pbwd(P, P, P, nmax_b + 1, l, None), b"too large")
        refused(bwd(P, P, P, 1 << 48, l, None), b"too large")
    refused(lib.lv_wigner_d_fwd(P, P, 1 << 48, 3, None), b"too large")
    for l in (0, 3, 20):
        assert fwd(P, P, 0, l, None) == 0
        assert bwd(P, P, P, 0, l, None) == 0
        assert pbwd(P, P, P, 0, l, None) == 0
        assert fwd(None, None, 0, l, None) == 0 and bwd(None, None, None, 0, l, None) == 0


def test_wigner_d_matrix_cpu_tensor_with_grad_fails_loudly():
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    a = torch.randn(4, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.wigner_d_matrix(a, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wigner_blocks(a, 2)
    with pytest.raises(AssertionError):
        lt.wigner_d_matrix(torch.randn(4, 2, requires_grad=True), 1)


@pytest.mark.parametrize("l", [0, 1, 2, 7, 20])
def test_k_formulas_match_oracle_autograd(l):
    """dD/dalpha = K D, dD/dgamma = D K, dD/dbeta = Xa J K Xb J Xc with K[i, 2l-i] = l - i
    (K = X^-1 dX/dtheta, the generator the kernel's xrot_dot_deriv products implement),
    against fp64 autograd through oracle.lie_ref.wigner_d: 1e-12 normwise per sample."""
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(100 + l)
    n, nn = 9, 2 * l + 1
    ang = (torch.rand(n, 3, generator=gen, dtype=torch.float64) * 2 - 1) * np.pi
    G = torch.randn(n, nn, nn, generator=gen, dtype=torch.float64)
    a = ang.clone().requires_grad_(True)
    (lie_ref.wigner_d(a, l) * G).sum().backward()
    K = torch.zeros(nn, nn, dtype=torch.float64)
    for i in range(nn):
        K[i, 2 * l - i] = l - i
    J = lie_ref.j_table(l).double()
    xa, xb, xc = (lie_ref.z_rotation(ang[:, i], l) for i in range(3))
    D = xa @ J @ xb @ J @ xc
    want = torch.stack([(G * (K @ D)).sum((1, 2)),
                        (G * (xa @ J @ K @ xb @ J @ xc)).sum((1, 2)),
                        (G * (D @ K)).sum((1, 2))], 1)
    got = a.grad
    err = (want - got).norm(dim=1) / got.norm(dim=1).clamp_min(1e-30)
    assert torch.isfinite(err).all() and err.max() <= 1e-12, (l, err.max().item())
    if l == 0:
        assert torch.equal(want, torch.zeros_like(want)) and torch.equal(got, torch.zeros_like(got))
