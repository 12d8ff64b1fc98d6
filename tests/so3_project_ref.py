"""Torch restatement of the SO(3) projection family (csrc/so3_device.h so3_project_*,
csrc/so3_stats.hip) in the dtype of its inputs: fp64 as the tests' yardstick,
fp32 to measure what the algorithm itself loses in that format.  The projection (Davenport's
q-method by cyclic Jacobi sweeps), its masked tangent-space backward, the weighted moment, the
chordal mean and the alternating two-sided alignment from four starts, with the seeded inputs
the CPU and GPU tests share.  Runs on any device-less machine; a test helper like
tests/so3_log_ref.py and tests/vmf_ref.py."""
import functools
import math

import torch

from so3_log_ref import hat, haar, log_polar

F64 = torch.float64
SWEEPS = {torch.float32: 6, F64: 8}            # so3_device.h project_sweeps<T>()
MASK = {torch.float32: 2.0 ** -12, F64: 2.0 ** -26}   # gamma <= sqrt(eps): gradient exactly 0
EPS = {torch.float32: 2.0 ** -24, F64: 2.0 ** -53}
PAIRS = ((0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2))   # round-robin: disjoint in twos
XT, YT, CT = 1, 2, 4                             # include/lievae.h LV_MOMENT_*


def vee2(X):
    """vee(X - X^T) = (X21 - X12, X02 - X20, X10 - X01)."""
    return torch.stack((X[..., 2, 1] - X[..., 1, 2], X[..., 0, 2] - X[..., 2, 0],
                        X[..., 1, 0] - X[..., 0, 1]), -1)


# ------------------------------------------------------------------ the projection
def _jacobi4(a, sweeps):
    """Cyclic Jacobi on symmetric 4x4 matrices held as a[p][q] lists of (...,) tensors:
    returns the diagonal and the eigenvector columns v[r][k]."""
    one, zero = torch.ones_like(a[0][0]), torch.zeros_like(a[0][0])
    v = [[one.clone() if r == k else zero.clone() for k in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            apq = a[p][q]
            nz = apq != 0
            d, b = a[q][q] - a[p][p], 2 * apq
            den = torch.maximum(d.abs() + torch.sqrt(d * d + b * b), b.abs())  # >= |b|, also when b^2 underflows
            t = b.abs() / torch.where(nz, den, one)
            t = torch.where((d >= 0) == (b >= 0), t, -t)
            t = torch.where(nz, t, zero)
            c = 1 / torch.sqrt(1 + t * t)
            s = t * c
            h = t * apq
            a[p][p], a[q][q] = a[p][p] - h, a[q][q] + h
            a[p][q] = a[q][p] = zero
            for r in range(4):
                if r != p and r != q:
                    arp, arq = a[r][p], a[r][q]
                    a[r][p] = a[p][r] = c * arp - s * arq
                    a[r][q] = a[q][r] = s * arp + c * arq
            for r in range(4):
                vrp, vrq = v[r][p], v[r][q]
                v[r][p] = c * vrp - s * vrq
                v[r][q] = s * vrp + c * vrq
    return [a[k][k] for k in range(4)], v


def project_full(M):
    """M (..., 3, 3) -> R (..., 3, 3), lam1, lam2: the nearest rotation and the two largest
    eigenvalues of Davenport's K (s1 = (lam1 + lam2)/2, s2 + s3' = (lam1 - lam2)/2, in units of
    the power of two M was scaled by).

    M is scaled by the power of two that brings its largest entry into [1/2, 1) (exact), K is
    built with the quaternion scalar-last, diagonalised by SWEEPS cyclic Jacobi sweeps; the
    eigenvector of the largest diagonal entry (ties: the scalar part first, so M = 0 gives I)
    is renormalised and turned into R."""
    mx = M.abs().flatten(-2).max(-1).values
    e = torch.frexp(mx)[1]
    # ldexp in two exact halves: torch forms 2^k in the dtype, which overflows for |k| > 127
    k = -e[..., None, None]
    k1 = torch.div(k, 2, rounding_mode="floor")
    m = torch.ldexp(torch.ldexp(M, k1), k - k1)
    m = [[m[..., i, j] for j in range(3)] for i in range(3)]
    tr = (m[0][0] + m[1][1]) + m[2][2]
    z = (m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1])
    a = [[None] * 4 for _ in range(4)]
    for i in range(3):
        for j in range(3):
            a[i][j] = (m[i][j] + m[j][i]) - tr if i == j else m[i][j] + m[j][i]
        a[i][3] = a[3][i] = z[i]
    a[3][3] = tr
    d, v = _jacobi4(a, SWEEPS[M.dtype])
    # top eigenvector, the scalar part preferred on ties
    k = torch.full_like(d[3], 3, dtype=torch.long)
    best = d[3]
    for i in range(3):
        up = d[i] > best
        best = torch.where(up, d[i], best)
        k = torch.where(up, torch.full_like(k, i), k)
    q = [torch.where(k == 0, v[r][0], torch.where(k == 1, v[r][1],
                                                  torch.where(k == 2, v[r][2], v[r][3])))
         for r in range(4)]
    lo01, hi01 = torch.minimum(d[0], d[1]), torch.maximum(d[0], d[1])
    lo23, hi23 = torch.minimum(d[2], d[3]), torch.maximum(d[2], d[3])
    lam2 = torch.maximum(torch.maximum(lo01, lo23), torch.minimum(hi01, hi23))
    nrm = torch.sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]))
    x, y, zz, w = (c / nrm for c in q)
    R = torch.stack([
        ((w * w + x * x) - y * y) - zz * zz, 2 * (x * y - w * zz), 2 * (x * zz + w * y),
        2 * (x * y + w * zz), ((w * w - x * x) + y * y) - zz * zz, 2 * (y * zz - w * x),
        2 * (x * zz - w * y), 2 * (y * zz + w * x), ((w * w - x * x) - y * y) + zz * zz], -1)
    return R.reshape(*M.shape), best, lam2


def project(M):
    return project_full(M)[0]


def gamma_of(M):
    """(s2 + s3') / s1 as the kernel sees it (NaN at M = 0)."""
    _, l1, l2 = project_full(M)
    return (l1 - l2) / (l1 + l2)


def _mm_tn(A, B):
    """A^T B entry by entry, summed left to right like so3_device.h matmul3_tn (torch's batched
    product rounds differently from host to host)."""
    return torch.stack([A[..., 0, i] * B[..., 0, j] + A[..., 1, i] * B[..., 1, j] + A[..., 2, i] * B[..., 2, j]
                        for i in range(3) for j in range(3)], -1).reshape(A.shape)


def _mul_hat(R, u):
    """R hat(u) entry by entry, like so3_device.h mul_hat."""
    u0, u1, u2 = u[..., 0, None], u[..., 1, None], u[..., 2, None]
    r0, r1, r2 = R[..., 0], R[..., 1], R[..., 2]
    return torch.stack([r1 * u2 - r2 * u1, r2 * u0 - r0 * u2, r0 * u1 - r1 * u0], -1)


def project_vjp(M, gR, fwd=None):
    """gM = R hat(u), A u = vee(R^T gR - gR^T R), A = tr(P) I - P, P = sym(R^T M), solved by
    cofactors; exactly 0 where gamma <= sqrt(eps) (MASK).  fwd: project_full(M), if at hand."""
    R, l1, l2 = project_full(M) if fwd is None else fwd
    keep = (l1 - l2) > MASK[M.dtype] * (l1 + l2)
    Q = _mm_tn(R, M)
    P = 0.5 * (Q + Q.transpose(-1, -2))
    tr = (P[..., 0, 0] + P[..., 1, 1]) + P[..., 2, 2]
    a, b, c = tr - P[..., 0, 0], -P[..., 0, 1], -P[..., 0, 2]
    d, e, f = tr - P[..., 1, 1], -P[..., 1, 2], tr - P[..., 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = (a * c00 + b * c01) + c * c02
    det = torch.where(keep, det, torch.ones_like(det))
    r = vee2(_mm_tn(R, gR))
    u = torch.stack([((c00 * r[..., 0] + c01 * r[..., 1]) + c02 * r[..., 2]) / det,
                     ((c01 * r[..., 0] + c11 * r[..., 1]) + c12 * r[..., 2]) / det,
                     ((c02 * r[..., 0] + c12 * r[..., 1]) + c22 * r[..., 2]) / det], -1)
    gM = _mul_hat(R, u)
    return torch.where(keep[..., None, None], gM, torch.zeros_like(gM))


class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M):
        ctx.save_for_backward(M)
        return project(M)

    @staticmethod
    def backward(ctx, g):
        (M,) = ctx.saved_tensors
        return project_vjp(M, g)


def project_ad(M):
    """project, differentiable with the masked tangent-space gradient."""
    return _Project.apply(M)


def svd_project(M):
    """U diag(1, 1, det UV^T) V^T in fp64: the independent yardstick."""
    U, _, Vh = torch.linalg.svd(M.double())
    d = torch.det(U @ Vh)
    D = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1))
    return U @ D @ Vh


def svd_gamma(M):
    s = torch.linalg.svdvals(M.double())
    sg = torch.where(torch.det(M.double()) < 0, -s[..., 2], s[..., 2])
    return (s[..., 1] + sg) / s[..., 0]


# ------------------------------------------------------------------ moment, mean, alignment
def moment(X, Y=None, w=None, C=None, flags=0):
    """S[s] = sum_i w_i op(X_i) C_s op(Y_i) in fp64, wsum, R[s] = project(S[s]) in X's dtype."""
    x = X.double().transpose(-1, -2) if flags & XT else X.double()
    ns = 1 if C is None else C.shape[0]
    if C is None:
        t = x[None]
    else:
        c = C.double().transpose(-1, -2) if flags & CT else C.double()
        t = x[None] @ c[:, None]
    if Y is not None:
        t = t @ (Y.double().transpose(-1, -2) if flags & YT else Y.double())[None]
    wd = torch.ones(X.shape[0], dtype=F64) if w is None else w.double()
    S = (wd[None, :, None, None] * t).sum(1)
    return S.reshape(ns, 3, 3), wd.sum(), project(S.reshape(ns, 3, 3)).to(X.dtype)


def so3_mean(R, weights=None):
    return moment(R, w=weights)[2][0]


def half_turn_starts(dtype):
    """The identity and the half-turns about x, y, z."""
    d = torch.tensor([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=dtype)
    return torch.diag_embed(d)


def align(Z, G, side="both", weights=None, rounds=16, starts=None):
    """(A, B, rms) with A G_i B ~ Z_i minimising sum w |Z_i - A G_i B|^2: one closed-form
    step for 'left' / 'right', `rounds` alternations from each start of B for 'both', the start
    of lowest residual kept.  rms = sqrt(residual / wsum)."""
    eye = torch.eye(3, dtype=Z.dtype)
    if side == "left":
        S, ws, R = moment(Z, G, weights, None, YT)
        A, B = R[0], eye
        res = 6 * ws - 2 * (A.double() * S[0]).sum()
    elif side == "right":
        S, ws, R = moment(G, Z, weights, None, XT)
        A, B = eye, R[0]
        res = 6 * ws - 2 * (B.double() * S[0]).sum()
    else:
        Bs = half_turn_starts(Z.dtype) if starts is None else starts
        for _ in range(rounds):
            As = moment(Z, G, weights, Bs, YT | CT)[2]
            S, ws, Bs = moment(G, Z, weights, As, XT | CT)
        res4 = 6 * ws - 2 * (Bs.double() * S).sum((-1, -2))
        k = torch.argmin(res4)
        A, B, res = As[k], Bs[k], res4[k]
    return A, B, torch.sqrt(res.clamp(min=0) / ws)


def kabsch(P, Q):
    """argmax over rotations R of tr(R^T sum_i P_i Q_i^T) by SVD, fp64."""
    return svd_project((P.double() @ Q.double().transpose(-1, -2)).sum(0))


def geodesic(A, B):
    return log_polar(A.transpose(-1, -2) @ B)[1]


# ------------------------------------------------------------------ shared inputs
FAMILY_N = 4099
FAMILIES = ("rot_1e-3", "rot_1", "rot_1e3", "noise_0.1", "noise_0.5", "gauss",
            "gap_1e-1_pos", "gap_1e-1_neg", "gap_1e-2_pos", "gap_1e-2_neg",
            "gap_1e-3_pos", "gap_1e-3_neg")


@functools.lru_cache(maxsize=None)
def family(name, n=FAMILY_N):
    """fp64 matrices of one input family (seeded, fixed)."""
    gen = torch.Generator().manual_seed(8100 + FAMILIES.index(name))
    kind, *rest = name.split("_")
    if kind == "rot":
        return haar(n, gen) * float(rest[0])
    if kind == "noise":
        return haar(n, gen) + float(rest[0]) * torch.randn(n, 3, 3, generator=gen, dtype=F64)
    if kind == "gauss":
        M = torch.randn(n, 3, 3, generator=gen, dtype=F64)
        want = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).to(F64)
        return M * (torch.sign(torch.det(M)) * want)[:, None, None]   # det M_i has sign (-1)^i
    g = float(rest[0])
    U, V = haar(n, gen), haar(n, gen)
    u = torch.rand(n, generator=gen, dtype=F64)
    if rest[1] == "pos":
        s3 = g * (0.05 + 0.45 * u)
        s2 = g - s3
    else:
        s3 = -(0.05 + 0.45 * u)
        s2 = g - s3
    one = torch.ones(n, dtype=F64)
    return U @ torch.diag_embed(torch.stack([one, s2, s3], -1)) @ V.transpose(-1, -2)


def rel_err(y, ref):
    return (y.double() - ref).flatten(1).norm(dim=-1) / ref.flatten(1).norm(dim=-1)


@functools.lru_cache(maxsize=None)
def family_case(name, dtype=torch.float32):
    """One family's input in `dtype`, the fp64 yardsticks on that same rounded input and the
    restatement's own error constants in `dtype` (computed once, shared, left unchanged):
      M, gR          the kernel's inputs
      R64, gM64      fp64 SVD projection / fp64 restatement backward
      gamma          (s2 + s3')/s1 by the fp64 SVD
      c_fwd, c_bwd   max over samples of err * gamma / eps of the restatement in `dtype`
                     (forward: |R - R64|_F; backward: |gM - gM64|_F / |gM64|_F).  In fp64
                     the backward has no yardstick of higher precision (gM64 is the fp64
                     restatement itself): its constant is the fp32 one of the same family --
                     the same operations in the same order lose the same multiples of eps
                     in either format
      orth, det      the restatement's worst |R^T R - I|_F and |det R - 1|."""
    M = family(name).to(dtype)
    gen = torch.Generator().manual_seed(8200 + FAMILIES.index(name))
    gR = torch.randn(M.shape[0], 3, 3, generator=gen, dtype=F64).to(dtype)
    R64 = svd_project(M)
    gamma = svd_gamma(M)
    assert (gamma > 5e-4).all(), name
    gM64 = project_vjp(M.double(), gR.double())
    fwd = project_full(M)
    R = fwd[0]
    gM = project_vjp(M, gR, fwd)
    eps = EPS[dtype]
    e_f = (R.double() - R64).flatten(1).norm(dim=-1)
    e_b = rel_err(gM, gM64)
    eye = torch.eye(3, dtype=F64)
    orth = ((R.double().transpose(-1, -2) @ R.double()) - eye).flatten(1).norm(dim=-1).max().item()
    det = (torch.det(R.double()) - 1).abs().max().item()
    c_bwd = float((e_b * gamma).max() / eps) if dtype != F64 else \
        family_case(name, torch.float32)["c_bwd"]
    return dict(M=M, gR=gR, R64=R64, gM64=gM64, gamma=gamma,
                c_fwd=float((e_f * gamma).max() / eps), c_bwd=c_bwd,
                orth=orth, det=det)


def singular_set(dtype=torch.float32):
    """Zero, rank 1, diag(1, 1, -1), a sample at gamma = 2^-13 (masked in fp32) and its
    neighbour at 2^-11 (not masked)."""
    gen = torch.Generator().manual_seed(8300)
    U, V = haar(2, gen), haar(2, gen)
    a = torch.randn(3, generator=gen, dtype=F64)
    b = torch.randn(3, generator=gen, dtype=F64)

    def gap(i, g):
        return U[i] @ torch.diag(torch.tensor([1.0, 0.5 + g, -0.5], dtype=F64)) @ V[i].T
    M = torch.stack([torch.zeros(3, 3, dtype=F64), torch.outer(a, b),
                     torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=F64)),
                     gap(0, 2.0 ** -13), gap(1, 2.0 ** -11)])
    return M.to(dtype)


def planted(n, angle_deg, noise, seed, dtype=F64):
    """Z_i = A0 G_i B0 exp(noise * xi_i) with the right factor B0 turned by `angle_deg`."""
    from so3_log_ref import exp
    gen = torch.Generator().manual_seed(seed)
    G = haar(n, gen)
    A0 = haar(1, gen)[0]
    ax = torch.randn(3, generator=gen, dtype=F64)
    B0 = exp(ax / ax.norm() * math.radians(angle_deg))
    Z = A0 @ G @ B0
    if noise > 0:
        Z = Z @ exp(noise * torch.randn(n, 3, generator=gen, dtype=F64))
    return Z.to(dtype), G.to(dtype), A0, B0


PLANTED_ANGLES = (30.0, 119.0, 121.0, 150.0, 179.0)
