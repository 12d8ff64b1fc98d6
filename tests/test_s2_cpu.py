"""CPU checks of the S^2 harmonics (csrc/s2.hip, lie_vae/s2.py): the numpy restatement the
GPU tests compare against (tests/s2_ref.py) is tied to scipy, to closed forms, to the package's
Wigner-D convention and to its own fp32 run; the quadrature grid is exact at and only at the
documented sizes; the launch plans and every argument check of the C entry points run without
a device; the Python API refuses CPU tensors."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import s2_ref as sr
from conftest import PKG_ROOT

LMAX = 20
LDS_PER_CU = 160 * 1024
LDS_NO_OPT_IN = 64 * 1024  # the kernels ask for no more than a launch gets without opting in
HARM, SYN, ANA = 0, 1, 2   # LV_S2_OP_*


def _points(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 3))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


POLES = np.array([[0, 0, 1.0], [0, 0, -1.0]])


# ------------------------------------------------------------------ the restatement
def test_restatement_matches_scipy():
    """Every degree l <= 20 against scipy's complex harmonics in gen_j's sign gauge (no
    Condon-Shortley phase, m < 0 sine-type), the poles included: <= 1e-10."""
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(PKG_ROOT, "tools"))
    try:
        import gen_j
    finally:
        sys.path.pop(0)
    # the poles themselves, but no point a hair off them: gen_j goes through arccos(z), which
    # loses half its digits there (the recurrence does not)
    x = np.concatenate([_points(200, 1), POLES])
    Y = sr.harmonics(x, LMAX)
    u = sr.unit(x)
    worst = 0.0
    for l in range(LMAX + 1):
        want = gen_j.real_sh(l, u.T).T
        worst = max(worst, np.abs(Y[:, l * l:(l + 1) ** 2] - want).max())
    print(f"restatement vs scipy, l <= {LMAX}: max abs {worst:.2e}")
    assert worst <= 1e-10


def test_closed_forms_and_poles():
    x = np.concatenate([_points(50, 2) * np.linspace(0.1, 9, 50)[:, None], POLES, 3 * POLES])
    u = x / np.linalg.norm(x, axis=1, keepdims=True)
    for dtype, tol in ((np.float64, 1e-15), (np.float32, 3e-7)):
        Y = sr.harmonics(x, LMAX, dtype)
        assert Y.dtype == dtype
        np.testing.assert_allclose(Y[:, 0], 1 / np.sqrt(4 * np.pi), rtol=0, atol=tol)
        c = np.sqrt(3 / (4 * np.pi))
        np.testing.assert_allclose(Y[:, 1:4], c * u[:, [1, 2, 0]], rtol=0, atol=tol)
        # at +-z every m != 0 entry is exactly zero, and m = 0 is sqrt((2l+1)/4pi) (+-1)^l
        for row, sign in ((-4, 1), (-3, -1), (-2, 1), (-1, -1)):
            for l in range(LMAX + 1):
                blk = Y[row, l * l:(l + 1) ** 2]
                assert np.all(np.delete(blk, l) == 0), (dtype, row, l)
                np.testing.assert_allclose(blk[l], np.sqrt((2 * l + 1) / (4 * np.pi)) * sign ** l,
                                           rtol=20 * tol, atol=0)
    # points without a direction: every entry NaN, the neighbours untouched
    bad = np.array([[0, 0, 0], [np.inf, 0, 1], [1, np.nan, 0], [0.3, 0.4, 0.5]])
    Y = sr.harmonics(bad, 3)
    assert np.isnan(Y[:3]).all() and np.isfinite(Y[3]).all()


def test_rotation_is_wigner_d():
    """Y_l(Rz(a) Ry(b) Rz(c) x) = D_l(a, b, c) Y_l(x), D_l = X(a) J X(b) J X(c) from the
    package's J tables: the convention the action kernels and the S^2 kernels share."""
    from lie_vae._jtab import j_numpy
    rng = np.random.default_rng(3)
    x = np.concatenate([_points(40, 4), POLES])
    Y = sr.harmonics(x, LMAX)
    angles = np.concatenate([rng.uniform(-np.pi, np.pi, (4, 3)),
                             [[0.3, 1e-4, -1.2], [2.0, np.pi - 1e-4, 0.5], [0, 0, 0]]])
    for a in angles:
        Yg = sr.harmonics(x @ sr.zyz(a).T, LMAX)
        for l in (1, 2, 5, 20):
            D = sr.wigner_d(a, l, j_numpy(l))
            err = np.abs(Yg[:, l * l:(l + 1) ** 2] - Y[:, l * l:(l + 1) ** 2] @ D.T).max()
            assert err <= 1e-9, (a, l, err)


def test_eazyz_gives_the_angles_of_the_transpose():
    """group_matrix_to_eazyz(R) (the oracle's mat_to_eazyz) returns (a, b, c) with
    Rz(a) Ry(b) Rz(c) = R^T, which is why synthesis(D(eazyz(R)) F, x) = synthesis(F, R x).
    fp32 angles: 5e-6 is a few roundings of an angle of size pi; a wrong side is O(1)."""
    from oracle import lie_ref
    torch.manual_seed(5)
    R = lie_ref.haar_matrices(64)
    ang = lie_ref.mat_to_eazyz(R).double().numpy()
    worst = 0.0
    for r, a in zip(R.double().numpy(), ang):
        worst = max(worst, np.abs(sr.zyz(a) - r.T).max())
    print(f"Rz Ry Rz of mat_to_eazyz(R) vs R^T: max abs {worst:.2e}")
    assert worst <= 5e-6


def test_grid_is_exact_only_at_the_documented_sizes():
    from lie_vae import s2
    L = LMAX

    def defect(nlat, nlon):
        x, w = sr.grid(L, nlat, nlon)
        Y = sr.harmonics(x, L)
        return np.abs(Y.T @ (Y * w[:, None]) - np.eye((L + 1) ** 2)).max()

    assert defect(L + 1, 2 * L + 1) <= 1e-12
    assert defect(L + 1, 2 * L) > 0.5
    assert defect(L, 2 * L + 1) > 0.5
    for nlat, nlon in ((L + 1, 2 * L), (L, 2 * L + 1)):
        with pytest.raises(ValueError, match="exactly"):
            s2.grid(L, nlat, nlon)
    x, w = s2.grid_numpy(6)
    xr, wr = sr.grid(6)
    np.testing.assert_allclose(x, xr, rtol=0, atol=1e-15)
    np.testing.assert_allclose(w, wr, rtol=1e-15, atol=0)
    assert abs(w.sum() - 4 * np.pi) < 1e-12
    xt, wt = s2.grid(6, 9, 16)
    assert xt.shape == (144, 3) and wt.shape == (144,) and xt.dtype == torch.float32
    e = s2.equirect_points(4, 8)
    assert e.shape == (32, 3) and e[0, 2] > 0 > e[-1, 2]
    np.testing.assert_allclose(e.norm(dim=1).numpy(), 1, atol=1e-6)
    th, ph = np.pi * 0.5 / 4, 2 * np.pi * 1.5 / 8
    np.testing.assert_allclose(e[1].numpy(), [np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph),
                                              np.cos(th)], atol=1e-7)


def test_fp32_restatement_is_a_quarter_of_the_gpu_bar():
    """What fp32 alone costs, on the very points of the GPU basis test: the fp32 run of the
    recurrence stays within 2.5e-6 of fp64, normwise per point (the GPU bar is 1e-5)."""
    worst = 0.0
    for L in sr.BASIS_DEGREES:
        for P in sr.BASIS_COUNTS:
            x = sr.basis_points(P)
            Y64, Y32 = sr.harmonics(x, L), sr.harmonics(x, L, np.float32)
            err = np.linalg.norm(Y32 - Y64, axis=1) / np.linalg.norm(Y64, axis=1)
            worst = max(worst, err.max())
    print(f"fp32 restatement vs fp64: max normwise error per point {worst:.2e}")
    assert worst <= 2.5e-6


def test_basis_points_hold_the_hard_cases():
    x = sr.basis_points(65)
    assert np.array_equal(x[0], [0, 0, 1]) and np.array_equal(x[1], [0, 0, -1])
    assert np.array_equal(x[6], np.float32([1e-4, 0, 1]))
    n = np.linalg.norm(x.astype(np.float64), axis=1)
    assert abs(n[7] - 1e-3) < 1e-9 and abs(n[8] - 1e3) < 1e-3
    assert np.array_equal(sr.basis_points(1)[0], [0, 0, 1])


# ------------------------------------------------------------------ plans
def _tile(C):
    return 1 if C <= 1 else 2 if C <= 2 else 4 if C <= 4 else 8 if C <= 8 else 16


def test_plans_over_the_whole_dispatch_space():
    from lie_vae import _lib
    lib = _lib.load()
    buf = (ctypes.c_int64 * 6)()
    tables = None
    for L in range(LMAX + 1):
        M = (L + 1) ** 2
        for C in range(1, 65):
            tile = _tile(C)
            ctiles = -(-C // tile)
            for P in (0, 1, 63, 64, 65, 4096):
                for B in (1, 3, 64):
                    assert lib.lv_s2_plan(SYN, B, P, L, C, buf) == 0
                    t, blocks, threads, lds, parts, red = buf
                    if tables is None:
                        tables = lds - M * tile * 4
                    small = P > 0 and B * ctiles * -(-P // 256) <= 512
                    assert t == tile and threads == (64 if small else 256)
                    assert blocks == B * ctiles * -(-P // threads) and (blocks >= 1) == (P > 0)
                    assert lds == tables + M * tile * 4 and lds <= LDS_NO_OPT_IN < LDS_PER_CU
                    assert parts == 0 and red == 0
                    assert lib.lv_s2_plan(ANA, B, P, L, C, buf) == 0
                    t, blocks, threads, lds, parts, red = buf
                    want = min(-(-P // 64), max(1, -(-2048 // (B * ctiles))))
                    assert t == tile and threads == 64 and lds == tables
                    assert parts == want and blocks == B * ctiles * parts
                    assert (blocks >= 1) == (P > 0) and (red >= 1) == (P > 0)
                    assert red == min(65536, -(-(B * M * C) // 256)) or P == 0
                    assert lib.lv_s2_analysis_workspace(B, P, L, C) == parts * B * M * C * 4
        for P in (0, 1, 63, 64, 65, 4096):
            assert lib.lv_s2_plan(HARM, 0, P, L, 0, buf) == 0
            assert tuple(buf) == (0, -(-P // 256), 256, tables, 0, 0)
    assert 1900 <= tables <= 2048  # 231 (A, B) pairs and 21 starts
    assert _lib.s2_plan(_lib.LV_S2_OP_SYNTHESIS, 64, 8192, 6, 10) == dict(
        tile=16, blocks=2048, threads=256, lds_bytes=tables + 49 * 16 * 4, partials=0,
        reduce_blocks=0)
    assert _lib.s2_plan(_lib.LV_S2_OP_ANALYSIS, 1, 8192, 20, 64)["partials"] == 128


def test_argument_checks_before_any_launch():
    """Every refusal of the header's contract returns LV_ERR_ARG with a message before
    anything is launched (dummy non-null pointers, no device); empty problems succeed."""
    from lie_vae import _lib
    lib = _lib.load()
    Q = ctypes.c_void_p(16)  # never dereferenced: the checks run first
    buf = (ctypes.c_int64 * 6)()
    big = 1 << 20

    def harm(x=Q, Y=Q, P=8, L=3):
        return lib.lv_s2_harmonics_fwd(x, Y, P, L, None)

    def syn(F=Q, stride=0, x=Q, out=Q, B=2, P=8, L=3, C=5):
        return lib.lv_s2_synthesis_fwd(F, stride, x, out, B, P, L, C, None)

    def ana(v=Q, x=Q, w=None, F=Q, B=2, P=8, L=3, C=5, ws=Q, nb=big):
        return lib.lv_s2_analysis_fwd(v, x, w, F, B, P, L, C, ws, nb, None)

    def refused(rc, word):
        msg = lib.lv_last_error()
        assert rc == -1 and msg and word in msg, (rc, msg)

    for L in (-1, 21):
        refused(harm(L=L), b"L must be")
        refused(syn(L=L), b"L must be")
        refused(ana(L=L), b"L must be")
        refused(lib.lv_s2_plan(SYN, 1, 8, L, 5, buf), b"L must be")
        assert lib.lv_s2_analysis_workspace(2, 8, L, 5) == 0
    for C in (0, 65, -3):
        refused(syn(C=C), b"C must be")
        refused(ana(C=C), b"C must be")
        refused(lib.lv_s2_plan(ANA, 1, 8, 3, C, buf), b"C must be")
    refused(harm(P=-1), b"P must be")
    refused(syn(P=-1), b"P must be")
    refused(ana(P=-1), b"P must be")
    refused(syn(B=-1), b"B must be")
    refused(ana(B=-1), b"B must be")
    refused(lib.lv_s2_plan(3, 1, 8, 3, 5, buf), b"op")
    refused(lib.lv_s2_plan(SYN, 1, 8, 3, 5, None), b"null")
    # null pointers with a non-empty problem
    refused(harm(x=None), b"null")
    refused(harm(Y=None), b"null")
    for kw in ("F", "x", "out"):
        refused(syn(**{kw: None}), b"null")
    for kw in ("v", "x", "F"):
        refused(ana(**{kw: None}), b"null")
    # the spectrum's batch stride: 0 or M * C only
    refused(syn(stride=79), b"F_batch_stride")
    assert syn(stride=80, B=0) == 0
    # a short or missing workspace
    need = lib.lv_s2_analysis_workspace(2, 8, 3, 5)
    assert need == 1 * 2 * 16 * 5 * 4
    refused(ana(nb=need - 1), b"workspace")
    refused(ana(ws=None), b"workspace")
    # sizes beyond the int64 byte range or the 2^31-1 block range
    refused(harm(P=1 << 61, L=20), b"range")
    refused(harm(P=1 << 55, L=0), b"blocks")
    refused(syn(B=1 << 40, P=1 << 40), b"range")
    refused(ana(B=1 << 40, P=1 << 40), b"range")
    refused(syn(B=1 << 30, P=1 << 12, C=64, L=0), b"blocks")
    refused(ana(B=1 << 57, P=1, L=0, C=1), b"blocks")
    assert lib.lv_s2_analysis_workspace(1 << 40, 1 << 40, 3, 5) == 0
    # empty problems succeed without pointers and launch nothing
    assert harm(x=None, Y=None, P=0) == 0
    assert syn(F=None, x=None, out=None, P=0) == 0
    assert syn(F=None, x=None, out=None, B=0) == 0
    assert ana(v=None, x=None, F=None, ws=None, nb=0, P=0) == 0
    assert ana(v=None, x=None, F=None, ws=None, nb=0, B=0) == 0
    assert lib.lv_s2_analysis_workspace(2, 0, 3, 5) == 0 == lib.lv_s2_analysis_workspace(0, 8, 3, 5)


# ------------------------------------------------------------------ the Python API
def test_python_api_refuses_cpu_tensors_and_bad_shapes():
    from lie_vae import s2
    from lie_vae.decoders import ActionNet
    x = torch.randn(7, 3)
    F = torch.randn(16, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s2.real_spherical_harmonics(x, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s2.synthesis(F, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s2.synthesis(F.expand(4, -1, -1), x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s2.analysis(torch.randn(7, 2), x, None, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s2.project(lambda p: p[:, 2:3], 3, "cpu")
    net = ActionNet(3, deconv=None, rep_copies=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.signal(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.signal(x, torch.randn(5, 3))
    with pytest.raises(AssertionError, match="3 dim vectors"):
        s2.real_spherical_harmonics(torch.randn(7, 2), 3)
    with pytest.raises(AssertionError, match="3 dim vectors"):
        s2.synthesis(F, torch.randn(7, 4))
    with pytest.raises(AssertionError, match=r"\(L\+1\)\^2"):
        s2.synthesis(torch.randn(15, 2), x)
    with pytest.raises(AssertionError, match="rows"):
        s2.analysis(torch.randn(6, 2), x, None, 3)
    with pytest.raises(AssertionError, match="weights"):
        s2.analysis(torch.randn(7, 2), x, torch.ones(6), 3)
