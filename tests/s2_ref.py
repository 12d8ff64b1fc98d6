"""numpy restatement of the S^2 kernels (csrc/s2.hip): the real spherical harmonics by the
pole-safe recurrence, synthesis, analysis and the Gauss-Legendre grid.  Everything runs in the
dtype asked for: fp64 is the reference the GPU tests compare against, fp32 shows what the
number format alone costs.  No scipy (the CPU tests compare this file against scipy where it
is installed).

Basis: orthonormal, real, no Condon-Shortley phase, flat index k = l^2 + l + m, m < 0
sine-type, m > 0 cosine-type:
    Y_l^{+-m}(x) = sqrt2 q_l^m(z) {Re, Im}(x + iy)^m,     Y_l^0 = q_l^0(z),
    q_m^m = sqrt((1/4pi) prod_{k<=m} (2k+1)/(2k)),
    q_l^m = A (z q_{l-1}^m - B q_{l-2}^m),  A = sqrt((4l^2-1)/(l^2-m^2)),
                                            B = sqrt(((l-1)^2-m^2)/(4(l-1)^2-1)),
with z q taken as +-(q - (1 - |z|) q) for |z| > 1/2 (see ``harmonics``).
"""
import numpy as np


def start(m):
    """q_m^m in fp64."""
    s = 0.25 / np.pi
    for k in range(1, m + 1):
        s *= (2.0 * k + 1.0) / (2.0 * k)
    return np.sqrt(s)


def unit(x, dtype=np.float64):
    """Directions of the points x (P,3), normalised in ``dtype`` the way the kernel does it
    (first by the largest component).  Points without a direction become NaN."""
    x = np.asarray(x, dtype=dtype)
    s = np.abs(x).max(axis=1, keepdims=True)
    ok = np.isfinite(x).all(axis=1, keepdims=True) & (s > 0)
    with np.errstate(all="ignore"):
        y = x / np.where(ok, s, 1)
        u = y / np.sqrt((y * y).sum(axis=1, keepdims=True, dtype=dtype))
    return np.where(ok, u, np.nan).astype(dtype)


def harmonics(x, L, dtype=np.float64):
    """x (P,3), any length -> Y (P,(L+1)^2) in ``dtype``; the recurrence's constants are
    computed in fp64 and rounded once."""
    u = unit(x, dtype)
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    P = u.shape[0]
    Y = np.zeros((P, (L + 1) ** 2), dtype=dtype)
    re, im = np.ones(P, dtype=dtype), np.zeros(P, dtype=dtype)
    bad = np.isnan(ux)
    # for |z| > 1/2 the product z q is +-(q - t q), t = 1 - |z| = (x^2 + y^2) / (1 + |z|), in
    # one rounding (the kernel's fmaf): a rounded z alone does not resolve the colatitude there
    with np.errstate(invalid="ignore"):
        t = ((ux * ux + uy * uy) / (dtype(1) + np.abs(uz))).astype(dtype)
        polar = np.abs(uz) > 0.5
    sign = np.where(uz < 0, dtype(-1), dtype(1))

    def zmul(q):
        if dtype == np.float32:  # products of two floats are exact in double: one rounding
            v = (q.astype(np.float64) - t.astype(np.float64) * q.astype(np.float64)).astype(dtype)
        else:
            v = q - t * q
        return np.where(polar, sign * v, uz * q)

    for m in range(L + 1):
        if m > 0:
            re, im = re * ux - im * uy, re * uy + im * ux
        q1 = np.full(P, dtype(start(m) * (np.sqrt(2.0) if m else 1.0)), dtype=dtype)
        q1[bad] = np.nan
        q2 = np.zeros(P, dtype=dtype)
        for l in range(m, L + 1):
            if l > m:
                a = dtype(np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m)))
                b = dtype(np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0)))
                q1, q2 = a * (zmul(q1) - b * q2), q1
            k0 = l * l + l
            if m == 0:
                Y[:, k0] = q1
            else:
                Y[:, k0 + m] = q1 * re
                Y[:, k0 - m] = q1 * im
    assert Y.dtype == dtype
    return Y


def synthesis(F, x, dtype=np.float64):
    """F (M,C) or (B,M,C), x (P,3) -> (P,C) or (B,P,C): values = Y F, all in ``dtype``."""
    F = np.asarray(F, dtype=dtype)
    L = int(round(np.sqrt(F.shape[-2]))) - 1
    return np.matmul(harmonics(x, L, dtype), F)


def analysis(values, x, w, L, dtype=np.float64):
    """values (P,C) or (B,P,C), x (P,3), w (P) or None -> (M,C) or (B,M,C):
    F = Y^T diag(w) values, all in ``dtype``."""
    values = np.asarray(values, dtype=dtype)
    Y = harmonics(x, L, dtype)
    if w is not None:
        Y = Y * np.asarray(w, dtype=dtype)[:, None]
    return np.matmul(Y.T, values)


def grid(L, nlat=None, nlon=None):
    """Gauss-Legendre nodes in z times equispaced longitudes, latitude-major, fp64:
    (x (nlat*nlon,3), w (nlat*nlon)), w = w_i 2 pi / nlon.  No size check (the CPU tests
    use the too-small grids on purpose)."""
    nlat = L + 1 if nlat is None else nlat
    nlon = 2 * L + 1 if nlon is None else nlon
    z, wz = np.polynomial.legendre.leggauss(nlat)
    phi = 2 * np.pi * np.arange(nlon) / nlon
    x = np.empty((nlat, nlon, 3))
    x[..., 0] = np.sqrt(1 - z * z)[:, None] * np.cos(phi)[None, :]
    x[..., 1] = np.sqrt(1 - z * z)[:, None] * np.sin(phi)[None, :]
    x[..., 2] = z[:, None]
    w = np.broadcast_to((wz * 2 * np.pi / nlon)[:, None], (nlat, nlon))
    return x.reshape(-1, 3), w.reshape(-1).copy()


# ------------------------------------------------------------------ rotations
def rz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def ry(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])


def zyz(a):
    """Rz(alpha) Ry(beta) Rz(gamma) in fp64 for a = (alpha, beta, gamma) of any float dtype."""
    al, be, ga = (float(v) for v in a)
    return rz(al) @ ry(be) @ rz(ga)


def z_rot(theta, l):
    """The matrix X(theta) of Y_l(Rz(theta) x) = X(theta) Y_l(x) in this basis (rows and
    columns m = -l..l): cos(m theta) on the diagonal, sin(-m theta) on the anti-diagonal."""
    n = 2 * l + 1
    freqs = np.arange(l, -l - 1, -1)
    m = np.zeros((n, n))
    m[np.arange(n), np.arange(n)[::-1]] = np.sin(freqs * theta)
    m[np.arange(n), np.arange(n)] = np.cos(freqs * theta)
    return m


def wigner_d(a, l, J):
    """D_l(alpha, beta, gamma) = X(alpha) J X(beta) J X(gamma) in fp64, J the degree's
    Pinchon-Hoggan matrix."""
    al, be, ga = (float(v) for v in a)
    return z_rot(al, l) @ J @ z_rot(be, l) @ J @ z_rot(ga, l)


# ------------------------------------------------------------------ shared test inputs
def basis_points(P, seed=0):
    """The points of the GPU basis test, fp32 (P,3): first the fixed hard cases -- the six
    axis directions, a point 1e-4 off the pole, lengths 1e-3 and 1e3 -- as far as P allows,
    then seeded random directions."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((2, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    fixed = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0],
                      [1e-4, 0, 1], 1e-3 * d[0], 1e3 * d[1]])
    pts = rng.standard_normal((P, 3))
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)
    n = min(P, len(fixed))
    # a single point keeps the pole; otherwise the hard cases come first
    pts[:n] = fixed[:n]
    return pts.astype(np.float32)


BASIS_DEGREES = (0, 1, 6, 20)
BASIS_COUNTS = (1, 63, 65, 257)
# (B, L, C, P) of the synthesis / analysis parity tests
TRANSFORM_SHAPES = ((1, 0, 1, 1), (1, 6, 10, 257), (3, 6, 10, 65), (2, 20, 3, 63), (1, 20, 64, 130))
