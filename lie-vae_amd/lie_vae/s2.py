"""Spherical harmonics on S^2: the signal behind the action decoder's spectrum (extension; the
reference only names it, "the virtual signal on the Sphere", experiments/main.py:169).

``item_rep`` is a ((L+1)^2, C) block of Fourier coefficients F.  ``synthesis`` evaluates
f(x) = sum_k F_k Y_k(x) at points of the sphere, ``analysis`` is its adjoint
F_k = sum_p w_p Y_k(x_p) f(x_p), and on a ``grid`` the two are inverse to each other for
band-limited signals.  All three run on the HIP kernels of csrc/s2.hip; there is no CPU path.

Basis: orthonormal real harmonics without the Condon-Shortley phase, flat index
k = l^2 + l + m with m < 0 sine-type and m > 0 cosine-type; Y_0 = 1/sqrt(4 pi), degree 1 is
sqrt(3/(4 pi)) (y, z, x).  It is the basis of the package's J tables: with
g = Rz(a) Ry(b) Rz(c), Y_l(g x) = wigner_d_matrix((a, b, c), l) Y_l(x), hence

    synthesis(block_wigner_matrix_multiply(angles, F, L), x) == synthesis(F, g^T x)

and, because ``group_matrix_to_eazyz(R)`` returns the angles of R^T, for a latent matrix R

    synthesis(D(group_matrix_to_eazyz(R)) F, x) == synthesis(F, R x)      (transpose=False)
                                                == synthesis(F, R^T x)    (transpose=True).

Points need not be unit vectors: the kernels normalise them.  The zero vector and points with
a non-finite component have no direction and give NaN.  Nothing here differentiates the
points or the quadrature weights.
"""
import numpy as np
import torch

from . import _ops


def _degrees(degrees):
    assert isinstance(degrees, int) and degrees >= 0, 'degrees must be a non-negative integer'
    return degrees


def real_spherical_harmonics(x, degrees):
    """x (...,3) -> Y (...,(degrees+1)^2), fp32.  Forward only: no gradient reaches x."""
    assert x.shape[-1] == 3, 'Input must be 3 dim vectors'
    L = _degrees(degrees)
    lead = x.shape[:-1]
    return _ops.s2_harmonics(x.reshape(-1, 3), L).reshape(*lead, (L + 1) ** 2)


def synthesis(spectrum, x):
    """The signal of ``spectrum`` at the points x (P,3): spectrum (M,C) -> (P,C); spectrum
    (B,M,C) -> (B,P,C), the points shared by the batch (a stride-0 expand of one (M,C) block
    is passed to the kernel once).  Differentiable in ``spectrum`` (the VJP is the analysis
    kernel with unit weights); the points are not differentiated."""
    assert x.dim() == 2 and x.shape[-1] == 3, 'Input must be 3 dim vectors'
    return _ops.s2_synthesis(spectrum, x)


def analysis(values, x, weights, degrees):
    """The adjoint of ``synthesis``: values (P,C) or (B,P,C) sampled at x (P,3), weights (P)
    or None (ones) -> spectrum (M,C) or (B,M,C), F_k = sum_p w_p Y_k(x_p) values_p.  With the
    points and weights of ``grid`` it inverts ``synthesis`` up to degree ``degrees``.
    Differentiable in ``values`` (the VJP is the synthesis kernel scaled by the weights);
    points and weights are not differentiated.  Bitwise reproducible."""
    assert x.dim() == 2 and x.shape[-1] == 3, 'Input must be 3 dim vectors'
    return _ops.s2_analysis(values, x, weights, _degrees(degrees))


def grid_numpy(degrees, nlat=None, nlon=None):
    """The quadrature of ``grid`` on the host in fp64: (x (nlat*nlon,3), w (nlat*nlon))."""
    L = _degrees(degrees)
    nlat = L + 1 if nlat is None else nlat
    nlon = 2 * L + 1 if nlon is None else nlon
    if nlat < L + 1 or nlon < 2 * L + 1:
        raise ValueError(f"grid: nlat >= {L + 1} and nlon >= {2 * L + 1} are needed for degree "
                         f"{L} (got {nlat}, {nlon}): below them the quadrature does not "
                         "integrate products of two harmonics exactly")
    z, wz = np.polynomial.legendre.leggauss(nlat)
    phi = 2 * np.pi * np.arange(nlon) / nlon
    s = np.sqrt((1 - z) * (1 + z))
    x = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)),
                  np.repeat(z[:, None], nlon, axis=1)], axis=-1).reshape(-1, 3)
    w = np.repeat(wz * (2 * np.pi / nlon), nlon)
    return x, w


def grid(degrees, nlat=None, nlon=None, device=None):
    """Gauss-Legendre nodes in z times equispaced longitudes, latitude-major: points
    (nlat*nlon,3) and weights w_i 2 pi / nlon, fp32 on ``device``, built on the host.  Exact
    for products of two harmonics of degree <= ``degrees`` iff nlat >= degrees+1 and
    nlon >= 2 degrees+1 (the defaults); anything smaller raises ValueError."""
    x, w = grid_numpy(degrees, nlat, nlon)
    return (torch.as_tensor(x, dtype=torch.float32).to(device),
            torch.as_tensor(w, dtype=torch.float32).to(device))


def equirect_points(height, width, device=None):
    """Pixel-centre directions of a (height, width) latitude-longitude image, row-major,
    (height*width,3): row i is the colatitude pi (i + 1/2) / height (north pole, +z, at the
    top), column j the longitude 2 pi (j + 1/2) / width."""
    assert height >= 1 and width >= 1, 'height and width must be positive'
    theta = np.pi * (np.arange(height) + 0.5) / height
    phi = 2 * np.pi * (np.arange(width) + 0.5) / width
    x = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.sin(theta), np.sin(phi)),
                  np.repeat(np.cos(theta)[:, None], width, axis=1)], axis=-1).reshape(-1, 3)
    return torch.as_tensor(x, dtype=torch.float32).to(device)


def project(fn, degrees, device):
    """The spectrum ((degrees+1)^2, C) of a callable fn(x (P,3)) -> (P,C) (or (P,)), by
    ``grid`` and ``analysis``; exact for a band-limited fn.  The result can be passed as
    ``ActionNet(item_rep=...)`` or as a ToyDataset spectrum."""
    x, w = grid(degrees, device=device)
    values = fn(x)
    if values.dim() == 1:
        values = values[:, None]
    assert values.dim() == 2 and values.shape[0] == x.shape[0], \
        f"project: fn must return ({x.shape[0]},C), got {tuple(values.shape)}"
    return analysis(values, x, w, degrees)
