"""numpy restatement of the triangle-mesh renderer of csrc/render_mesh.hip,
packing and tracing, fp64 by default, operation for operation in the kernel's order, with the
per-pixel edge mask the comparisons need.

Camera, sub-sample positions, light and the pixel mean are those of tests/spherecube_ref.py
(and are imported from it).  A ray walks the triangles in index order; Moeller-Trumbore with
every dot product as (a0 b0 + a1 b1) + a2 b2; two-sided flat shading from the packed record.

A ray within a rounding of a silhouette or of an edge between two triangles may land on either
side of it, so ``render`` also returns a mask of the pixels with a sub-sample whose hit
triangle id (-1 for the background) changes when the sample moves by +-EDGE_SHIFT pixel in x
or in y; value comparisons leave those pixels out and assert that they are few (MASK_CAP).
"""
import numpy as np

import spherecube_ref as sr
from spherecube_ref import EDGE_SHIFT, MASK_CAP, _positions, haar_poses, off_edge_error  # noqa: F401

AMBIENT, DIFFUSE = sr.AMBIENT, sr.DIFFUSE
NO_HIT = -1


def _dot(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def pack(vertices, faces, albedo, dtype=np.float64, round32=True):
    """Records (T,16) of ``dtype`` from vertices (V,3), faces (T,3) and albedo (T,3); and the
    number of triangles with an index outside [0, V), whose records are zero.  Vertices and
    albedo are rounded to fp32 first, the values the device holds (round32=False keeps them:
    for comparisons with another fp64 scene)."""
    f = dtype
    first = np.float32 if round32 else np.float64
    v = np.asarray(vertices, dtype=first).reshape(-1, 3).astype(f)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    alb = np.asarray(albedo, dtype=first).reshape(-1, 3).astype(f)
    T, V = faces.shape[0], v.shape[0]
    rec = np.zeros((T, 16), dtype=f)
    ok = ((faces >= 0) & (faces < V)).all(axis=1)
    fi = np.where(ok[:, None], faces, 0) if V else np.zeros_like(faces)
    if V == 0 or T == 0:
        return rec, int((~ok).sum())
    v0 = v[fi[:, 0]]
    with np.errstate(all="ignore"):
        e1, e2 = v[fi[:, 1]] - v0, v[fi[:, 2]] - v0
        c0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        c1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        c2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        ln = np.sqrt(_dot(c0, c1, c2, c0, c1, c2))
        light = sr.LIGHT.astype(f)
        nl = _dot(c0 / ln, c1 / ln, c2 / ln, light[0], light[1], light[2])
        # fmax / fmin drop a NaN, as fmaxf / fminf do
        nf = np.fmin(np.fmax(nl, f(0)), f(1))
        nb = np.fmin(np.fmax(-nl, f(0)), f(1))
        solid = (ln > 0) & (ln < np.inf)
        alb = np.fmin(np.fmax(alb, f(0)), f(1))
        front = np.where(solid[:, None], alb * (f(AMBIENT) + f(DIFFUSE) * nf)[:, None], f(0))
        back = np.where(solid[:, None], alb * (f(AMBIENT) + f(DIFFUSE) * nb)[:, None], f(0))
    # without a finite positive area the edges are zeroed too: det == 0 exactly, never hit
    e1, e2 = np.where(solid[:, None], e1, f(0)), np.where(solid[:, None], e2, f(0))
    full = np.concatenate([v0, e1, e2, front, back, np.zeros((T, 1), dtype=f)], axis=1)
    rec[ok] = full[ok]
    return rec, int((~ok).sum())


def trace(R, rec, kx, ky, size, dtype=np.float64):
    """Colours (n, P, 3) and hit triangle ids (n, P) (NO_HIT: background) of the rays through
    the image-plane positions (kx, ky) (pixel units, P values) for the poses R (n,3,3)."""
    f = dtype
    R = np.asarray(R, dtype=f)
    rec = np.asarray(rec, dtype=f)
    kx, ky = np.asarray(kx, dtype=f), np.asarray(ky, dtype=f)
    u = ((kx / f(size) - f(0.5)) * f(2 * sr.TAU))[None, :]
    v = ((f(0.5) - ky / f(size)) * f(2 * sr.TAU))[None, :]
    o = f(sr.CAM_DIST) * R[:, :, 2]                                   # (n, 3)
    d = [(u * R[:, k, 0, None] + v * R[:, k, 1, None]) - R[:, k, 2, None] for k in range(3)]
    n, P = R.shape[0], kx.shape[0]
    best = np.full((n, P), np.inf, dtype=f)
    hit_id = np.full((n, P), NO_HIT, dtype=np.int64)
    col = np.zeros((n, P, 3), dtype=f)
    with np.errstate(all="ignore"):
        for k in range(rec.shape[0]):
            r = rec[k]
            v0, e1, e2, front, back = r[0:3], r[3:6], r[6:9], r[9:12], r[12:15]
            p0 = d[1] * e2[2] - d[2] * e2[1]
            p1 = d[2] * e2[0] - d[0] * e2[2]
            p2 = d[0] * e2[1] - d[1] * e2[0]
            det = _dot(p0, p1, p2, e1[0], e1[1], e1[2])
            inv = f(1) / det
            s0, s1, s2 = ((o[:, a] - v0[a])[:, None] for a in range(3))
            uu = _dot(s0, s1, s2, p0, p1, p2) * inv
            q0 = s1 * e1[2] - s2 * e1[1]
            q1 = s2 * e1[0] - s0 * e1[2]
            q2 = s0 * e1[1] - s1 * e1[0]
            vv = _dot(d[0], d[1], d[2], q0, q1, q2) * inv
            t = _dot(q0, q1, q2, e2[0], e2[1], e2[2]) * inv
            hit = (det != 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > 0) & (t < best)
            best = np.where(hit, t, best)
            hit_id = np.where(hit, k, hit_id)
            col = np.where(hit[..., None], np.where((det > 0)[..., None], front, back), col)
    return col, hit_id


def render(R, rec, size=64, samples=2, rgb=True, dtype=np.float64, mask=True):
    """Images (n, 3 | 1, size, size) of the records ``rec`` (from ``pack`` in the same
    ``dtype``) and the edge mask (n, size, size), True = leave out (None with mask=False; the
    mask is always traced in fp64, from the records given)."""
    f = dtype
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    n, S = R.shape[0], samples
    ky, kx = _positions(size, S, f)
    col, _ = trace(R, rec, kx, ky, size, f)
    col = col.reshape(n, size, S, size, S, 3)
    acc = np.zeros((n, size, size, 3), dtype=f)
    for a in range(S):            # the kernel's order: rows of sub-samples, then columns
        for b in range(S):
            acc = acc + col[:, :, a, :, b, :]
    img = np.moveaxis(acc / f(S * S), -1, 1)
    if not rgb:
        img = (((img[:, 0] + img[:, 1]) + img[:, 2]) / f(3))[:, None]
    img = np.ascontiguousarray(img)
    if not mask:
        return img, None
    return img, edge_mask(R, rec, size, S)


def edge_mask(R, rec, size, samples):
    """(n, size, size): pixels with a sub-sample whose fp64 hit id changes under a shift of
    +-EDGE_SHIFT pixel in x or in y."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    rec = np.asarray(rec, dtype=np.float64)
    ky, kx = _positions(size, samples, np.float64)
    _, hit0 = trace(R, rec, kx, ky, size)
    edge = np.zeros(hit0.shape, dtype=bool)
    for dx, dy in ((EDGE_SHIFT, 0), (-EDGE_SHIFT, 0), (0, EDGE_SHIFT), (0, -EDGE_SHIFT)):
        _, h = trace(R, rec, kx + dx, ky + dy, size)
        edge |= h != hit0
    return edge.reshape(R.shape[0], size, samples, size, samples).any(axis=(2, 4))


# ------------------------------------------------------------------ the compared cases
def soup(T, seed):
    """A random two-sided triangle soup: T triangles of edge about 0.8 with centres in a ball
    of radius about 1, windings random, one albedo per triangle.  (vertices, faces, albedo)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((T, 1, 3)) * 0.55
    v = (c + rng.standard_normal((T, 3, 3)) * 0.35).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * T).reshape(T, 3)
    albedo = rng.uniform(0.1, 1.0, (T, 3)).astype(np.float32)
    return v, faces, albedo


SOUP_SIZES = (63, 64, 65, 257)
QUARTER_TURN_CASES = ("cube 64x64 S=2 rgb", "icosahedron 12x12 S=4 rgb")


def parity_cases():
    """name -> (mesh builder name or ("soup", T, seed), R (n,3,3) fp64, size, samples, rgb):
    the cases the device is compared on.  The seeds are chosen so that each case's edge mask
    stays under MASK_CAP; tests/test_mesh_cpu.py asserts that."""
    cases = {
        "cube 64x64 S=2 rgb": ("cube", sr.parity_cases()["64x64 S=2 rgb"][0], 64, 2, True),
        "icosahedron 16x16 S=2 rgb": ("icosahedron", haar_poses(4, 10), 16, 2, True),
        "icosahedron 7x7 S=3 rgb": ("icosahedron", haar_poses(3, 11), 7, 3, True),
        "icosahedron 12x12 S=4 rgb": ("icosahedron", haar_poses(2, 12), 12, 4, True),
        "icosahedron 8x8 S=1 grey": ("icosahedron", haar_poses(3, 13), 8, 1, False),
        "icosphere2 32x32 S=2 rgb": ("icosphere2", haar_poses(2, 14), 32, 2, True),
        "triangle 16x16 S=2 rgb": ("triangle", np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0])]), 16, 2, True),
    }
    for T in SOUP_SIZES:
        cases[f"soup{T} 16x16 S=2 rgb"] = (("soup", T, SOUP_SEEDS[T]), haar_poses(2, 20 + T), 16, 2, True)
    return cases


SOUP_SEEDS = {63: 0, 64: 0, 65: 0, 257: 0}

# one large triangle in the plane z = 0.25, wound so that its normal is +z: the identity pose
# (camera on +z) sees its front, the half turn about x (camera on -z) its back
TRIANGLE = (np.array([(-1.5, -1.2, 0.25), (1.6, -0.9, 0.25), (0.1, 1.5, 0.25)], dtype=np.float32),
            np.array([(0, 1, 2)]), np.array([(0.9, 0.6, 0.3)], dtype=np.float32))


def case_arrays(spec):
    """(vertices, faces, albedo) of a parity case's mesh."""
    if isinstance(spec, tuple):
        return soup(spec[1], spec[2])
    if spec == "triangle":
        return TRIANGLE
    from lie_vae import meshes
    m = {"cube": meshes.cube, "icosahedron": lambda: meshes.icosahedron().normalized(1.5),
         "icosphere2": lambda: meshes.icosphere(2).normalized(1.5)}[spec]()
    return m.vertices, m.faces, m.albedo


def cube_anchor():
    """The comparison that ties this restatement to tests/spherecube_ref.py: the 12 poses of the
    sphere-cube parity case "64x64 S=2 rgb" (as the device sees them), the sphere-cube scene's
    fp64 image, the fp64 image of ``meshes.cube()`` and the pixels to compare: those without a
    sub-sample on the sphere and outside both edge masks.  (R, sc_img, cube_img, keep)."""
    R, size, S, rgb = sr.parity_cases()["64x64 S=2 rgb"]
    R = R.astype(np.float32).astype(np.float64)
    sc_img, sc_mask = sr.render(R, size, S, rgb)
    ky, kx = _positions(size, S, np.float64)
    _, hit = sr.trace(R, kx, ky, size)
    on_sphere = (hit == sr.ID_SPHERE).reshape(len(R), size, S, size, S).any(axis=(2, 4))
    v, faces, _ = case_arrays("cube")
    rec, _ = pack(v, faces, np.repeat(np.asarray(sr.FACE_ALBEDO), 2, axis=0), round32=False)
    cube_img, cube_mask = render(R, rec, size, S, rgb)
    return R, sc_img, cube_img, ~(on_sphere | sc_mask | cube_mask)
