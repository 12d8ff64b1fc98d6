"""SO(3) tools — drop-in for ``lie_vae.lie_tools`` (reference ``lie_vae/lie_tools.py``).

Same names, argument meaning and shape asserts as the reference; the numerical work
runs in the HIP kernels of ``liblievae_hip.so`` (fp32; the Gram–Schmidt map in fp64 as
in the reference).  Inputs must live on a HIP device — there is no CPU fallback.
Pure data rearrangements (hat/vee) and the RNG-driven samplers stay tensor ops on
whatever device the caller uses.
"""
import math
from functools import lru_cache

import numpy as np
import torch

from . import _ops
from ._jtab import j_numpy

__all__ = [
    "j_matrix", "map_to_lie_algebra", "map_to_lie_vector", "rodrigues", "s2s1rodrigues",
    "s2s2_gram_schmidt", "vector_to_eazyz", "log_map", "group_matrix_to_quaternions",
    "quaternions_to_eazyz", "group_matrix_to_eazyz", "quaternions_to_group_matrix",
    "wigner_d_matrix", "block_wigner_matrix_multiply", "random_quaternions",
    "random_group_matrices", "so3_log", "geodesic_distance", "project_to_so3", "so3_mean",
    "align_rotations", "render_spherecube", "render_mesh",
]


@lru_cache(maxsize=256)
def j_matrix(l, device=None):
    """J_l (fp32) — reference lie_tools.py:10-14 (lie_learn Jd, regenerated here)."""
    return torch.tensor(j_numpy(l), dtype=torch.float32, device=torch.device(device or "cpu"))


def map_to_lie_algebra(v):
    """hat: (...,3) -> (...,3,3) — lie_tools.py:17-43."""
    assert v.size()[-1] == 3
    z = torch.zeros_like(v[..., 0])
    x, y, w = v[..., 0], v[..., 1], v[..., 2]
    return torch.stack([z, -w, y, w, z, -x, -y, x, z], -1).reshape(*v.shape[:-1], 3, 3)


def map_to_lie_vector(X):
    """vee — lie_tools.py:46-53."""
    return torch.stack((-X[..., 1, 2], X[..., 0, 2], -X[..., 0, 1]), -1)


def rodrigues(v):
    """so(3) exp, (...,3) -> (...,3,3) — lie_tools.py:56-64 (NaN at |v| = 0, as there)."""
    assert v.shape[-1] == 3
    return _ops.unary(v, _ops.SO3_EXP)


def s2s1rodrigues(s2_el, s1_el):
    """lie_tools.py:67-78."""
    return _ops.s2s1(s2_el, s1_el)


def s2s2_gram_schmidt(v1, v2):
    """lie_tools.py:81-89, fp64 like S2S2Mean (cross along the last axis)."""
    out = _ops.s2s2(v1, v2)
    return out if v1.dtype == torch.float64 else out.to(v1.dtype)


def vector_to_eazyz(v):
    """tanh squashing to ZYZ ranges — lie_tools.py:92-97 (latent modes normal/vmf)."""
    angles = torch.tanh(v) * v.new_tensor([math.pi, math.pi / 2, math.pi])
    return angles + v.new_tensor([0, math.pi / 2, 0])


def log_map(R):
    """Log map to skew matrices — lie_tools.py:100-109.

    A single (3,3) matrix keeps the reference's tensor expression (a test helper there:
    ``torch.trace`` makes it unbatched; NaN at the identity, no digits near π), on any device.
    Input with leading dimensions, which the reference raises on, goes through the HIP kernel:
    ``map_to_lie_algebra(so3_log(R))``, (...,3,3)."""
    if R.dim() > 2:
        return map_to_lie_algebra(so3_log(R))
    anti_sym = .5 * (R - R.transpose(-1, -2))
    theta = torch.acos(.5 * (torch.trace(R) - 1))
    return theta / torch.sin(theta) * anti_sym


def so3_log(R):
    """so(3) log, (...,3,3) rotations -> (...,3) with |v| ∈ [0, π]; the inverse of ``rodrigues``.

    Stable over the whole range (the identity gives exactly 0; near π the axis comes from the
    symmetric part of R) and differentiable with the tangent-space gradient R·hat(u)
    (include/lievae.h).  At exactly π the axis' largest component is positive.  Extension:
    the reference has only the unbatched ``log_map``."""
    assert list(R.shape[-2:]) == [3, 3], 'Input must be 3x3 matrices'
    return _ops.unary(R, _ops.SO3_LOG)


def geodesic_distance(A, B):
    """Rotation angle of AᵀB, (...,3,3) × (...,3,3) of one shape -> (...) in [0, π]: the
    geodesic distance on SO(3).  Differentiable in both (gradient 0 where the distance is 0).
    Extension."""
    assert list(A.shape[-2:]) == [3, 3] and list(B.shape[-2:]) == [3, 3], \
        'Input must be 3x3 matrices'
    return _ops.so3_angle(A, B)


def project_to_so3(M):
    """Nearest rotation in the Frobenius norm, (...,3,3) -> (...,3,3): the orthogonal Procrustes
    projection U·diag(1, 1, det UVᵀ)·Vᵀ of M = U·diag(s)·Vᵀ, in one kernel (Davenport's q-method;
    include/lievae.h lv_so3_project_fwd) without forming U or V.  fp32 or fp64 following the
    input.  Differentiable with the tangent-space gradient R·hat(u); where the gap
    (s2 + s3')/s1 is below √eps the sample's gradient is exactly 0.  Every finite M gives a
    rotation.  Extension: not in the reference."""
    assert list(M.shape[-2:]) == [3, 3], 'Input must be 3x3 matrices'
    return _ops.unary(M, _ops.SO3_PROJECT)


def so3_mean(R, weights=None):
    """Chordal (projected arithmetic) mean of rotations, (n,3,3) [, weights (n)] -> (3,3): a
    deterministic fp64 reduction and its projection (lv_so3_moment).  Forward only.
    Extension."""
    assert R.dim() == 3 and list(R.shape[-2:]) == [3, 3], 'Input must be (n,3,3)'
    return _ops.so3_mean(R, weights)


def align_rotations(Z, G, side='both', weights=None, rounds=16):
    """Rotations (A, B) and the rms residual with A·G_i·B ≈ Z_i in the least-squares (chordal)
    sense; Z, G (n,3,3).  ``side='left'`` fixes B = I, ``'right'`` fixes A = I (closed-form
    Procrustes steps); ``'both'`` alternates them ``rounds`` times from four starts of B (the
    identity and the three coordinate half-turns: one is always within 120° of the optimum)
    and keeps the best.  No host synchronisation; forward only.  Extension: the latent of an
    action-decoder VAE is identified only up to such a pair."""
    return _ops.align_rotations(Z, G, side=side, weights=weights, rounds=rounds)


def render_spherecube(g, size=64, rgb=True, samples=2):
    """Images (n, 3 | 1, size, size) of the sphere-cube scene seen from the camera frames g,
    matrices (n,3,3) or scalar-last quaternions (n,4), rendered on g's device in one kernel
    (include/lievae.h lv_render_spherecube_fwd; the scene: DESIGN.md §4.9).  ``g·Rz(φ)``
    rotates the image in plane.  Forward only.  Extension: the reference reads these images
    from files that Blender rendered."""
    return _ops.render_spherecube(g, size=size, rgb=rgb, samples=samples)


def render_mesh(g, meshes, mesh_id=None, size=64, rgb=True, samples=2):
    """Images (n, 3 | 1, size, size) of triangle meshes seen from the camera frames g, matrices
    (n,3,3) or scalar-last quaternions (n,4), rendered on g's device in one kernel
    (include/lievae.h lv_render_mesh_fwd) with render_spherecube's camera and
    light.  ``meshes``: a meshes.MeshSet on g's device, or a meshes.Mesh, which is packed on
    the fly (a host sync; pack once into a MeshSet to avoid it).  ``mesh_id`` (n,) integers
    picks each image's mesh (None: mesh 0; an id outside the set renders the background).
    Forward only.  Extension: the reference reads such images from files."""
    from .meshes import Mesh, MeshSet
    if isinstance(meshes, Mesh):
        _ops._lib.require_device(g)
        meshes = MeshSet([meshes], g.device)
    return _ops.render_mesh(g, meshes, mesh_id, size=size, rgb=rgb, samples=samples)


def group_matrix_to_quaternions(r):
    """Scalar-last quaternions — lie_tools.py:112-157."""
    assert list(r.shape[-2:]) == [3, 3], 'Input must be 3x3 matrices'
    return _ops.unary(r, _ops.MAT_TO_QUAT)


def quaternions_to_eazyz(q):
    """ZYZ Euler angles, not mod 2π — lie_tools.py:160-175."""
    assert q.shape[-1] == 4, 'Input must be 4 dim vectors'
    return _ops.unary(q, _ops.QUAT_TO_EAZYZ)


def group_matrix_to_eazyz(r):
    """lie_tools.py:178-180 (one fused kernel)."""
    assert list(r.shape[-2:]) == [3, 3], 'Input must be 3x3 matrices'
    return _ops.unary(r, _ops.MAT_TO_EAZYZ)


def quaternions_to_group_matrix(q):
    """Normalises q — lie_tools.py:183-192."""
    assert q.shape[-1] == 4
    return _ops.unary(q, _ops.QUAT_TO_MAT)


def wigner_d_matrix(angles, degree):
    """D_l(α,β,γ) = X(α)·J·X(β)·J·X(γ), (...,3) -> (...,2l+1,2l+1) — lie_tools.py:211-223.

    Materialises D_l in one launch (the decoder path never forms D) and is differentiable
    in the angles, like the reference's tensor expression; fp32 for any input dtype."""
    assert angles.shape[-1] == 3, 'Input must be 3 dim vectors'
    lead = angles.shape[:-1]
    n = 2 * degree + 1
    return _ops.wigner_block(angles.reshape(-1, 3), degree).reshape(*lead, n, n)


def block_wigner_matrix_multiply(angles, spectrum, max_degree, transpose=False):
    """Block-diagonal D(g)·F for l = 0..max_degree — lie_tools.py:226-253.

    angles (batch, 3); spectrum (batch, (L+1)^2, C), a stride-0 expand of a
    ((L+1)^2, C) tensor (shared, as ActionNet passes it) or a per-sample tensor.
    Output (batch, (L+1)^2, C)."""
    return _ops.group_action(angles, spectrum, max_degree, transpose=transpose)


def random_quaternions(n, dtype=torch.float32, device=None, generator=None):
    """Haar-uniform quaternions (Shoemake) — lie_tools.py:256-263.  ``generator`` (extension):
    a torch.Generator of ``device`` to draw from instead of the device's default stream."""
    u1, u2, u3 = torch.rand(3, n, dtype=dtype, device=device, generator=generator)
    return torch.stack((
        torch.sqrt(1 - u1) * torch.sin(2 * np.pi * u2),
        torch.sqrt(1 - u1) * torch.cos(2 * np.pi * u2),
        torch.sqrt(u1) * torch.sin(2 * np.pi * u3),
        torch.sqrt(u1) * torch.cos(2 * np.pi * u3),
    ), 1)


def random_group_matrices(n, dtype=torch.float32, device=None, generator=None):
    """lie_tools.py:266-267."""
    return quaternions_to_group_matrix(random_quaternions(n, dtype, device, generator))
